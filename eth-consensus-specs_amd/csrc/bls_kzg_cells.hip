// Fulu cell KZG kernels (specs/fulu/polynomial-commitments-sampling.md; the transform's pieces and index maps are in
// bls_fr_ntt.h, the field in bls_fr.h; C ABI: bls_capi_kzg_cells.hip).
//
//   k_ntt_tables       W[i] = w^i, 7^i, 7^-i (3 x 8,192 entries), once per context
//   k_ntt_pass1 / 2    the four-step transform of 4,096 or 8,192 points per blob: a workgroup of 256 lanes does four
//                      sub-transforms of 64 or 128 points, one per wave, each in its own 4 KB of LDS
//   k_cells_scatter    the present cells' bytes -> elements at their places of the extended blob, < r verdicts
//   k_cells_vanish     recovery's vanishing polynomial: its 128 values on the domain, its 128 inverses on the coset
//   k_cells_pointwise  dst[i] = src[i or brp13(i)] mul[i mod m]: the products and the 7^(+-i) scalings of recovery
//   k_fr_encode        elements -> 32 big-endian bytes
// Verification of cells against commitments and proofs:
//   k_cells_interp     a cell's bytes -> the 64 coefficients of its interpolation polynomial, one wave per cell
//                      (the inverse 64-point sub-transform in 2 KB of LDS, then the h_k^-m / 64 scaling), < r verdict
//   k_cells_rlc        the batch's r_k, the proofs' scalar rows r_k h_k^64 and r_k, the proofs' second copies
//   k_cells_weights    the commitments' scalar rows sum_{k: commitment of k = i} r_k
//   k_cells_colsum     s_m = sum_k r_k c_{k,m} in two levels (partials of 64 cells, then their sum); row m = -s_m
//   k_cells_put        the interpolants' sum (one row of the table MSM) into its place among the scaled points
//   k_cells_item_pairs every item's own two pairs (after a failed batch check)
#include "bls_kernels.h"
#include "bls_curve.h"
#include "bls_fr_ntt.h"
#include "bls_sha256.h"

namespace bls {

namespace {
inline unsigned nblk(size_t n, unsigned t) { return (unsigned)((n + t - 1) / t); }
constexpr uint32_t NTT_WG = 256, NTT_WAVES = 4;
}  // namespace

__global__ void __launch_bounds__(256) k_ntt_tables(Fr* tab) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 3 * NTT_EXT) tab[i] = ntt_table_entry(i);
}

// sub-transform `sub` of `total`: blob sub / 64, column sub mod 64
__global__ void __launch_bounds__(256) k_ntt_pass1(const Fr* src, size_t src_stride, Fr* tmp, const Fr* W,
                                                   uint32_t logn, uint32_t flags, uint32_t limit, uint32_t total) {
  __shared__ Fr sh[NTT_WAVES][NTT_SUB_MAX];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t sub = blockIdx.x * NTT_WAVES + wave;
  const bool active = sub < total;
  const size_t b = sub >> 6;
  const uint32_t c = sub & 63, logn1 = logn - 6;
  Fr* buf = sh[wave];
  if (active) ntt_p1_load(src + b * src_stride, buf, logn, flags, limit, c, lane, 64);
  __syncthreads();
#pragma unroll 1
  for (uint32_t s = 1; s <= logn1; ++s) {
    if (active) ntt_sub_stage(buf, logn1, s, W, (flags & NTT_INV) != 0, lane, 64);
    __syncthreads();
  }
  if (active) ntt_p1_store(buf, tmp + (b << logn), logn, flags, W, c, lane, 64);
}

// sub-transform `sub` of `total`: blob sub / n1, row sub mod n1
__global__ void __launch_bounds__(256) k_ntt_pass2(const Fr* tmp, Fr* dst, size_t dst_stride, const Fr* W,
                                                   uint32_t logn, uint32_t flags, uint32_t total) {
  __shared__ Fr sh[NTT_WAVES][64];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t sub = blockIdx.x * NTT_WAVES + wave;
  const bool active = sub < total;
  const uint32_t logn1 = logn - 6;
  const size_t b = sub >> logn1;
  const uint32_t k1 = sub & ((1u << logn1) - 1);
  Fr* buf = sh[wave];
  if (active) ntt_p2_load(tmp + (b << logn), buf, k1, lane, 64);
  __syncthreads();
#pragma unroll 1
  for (uint32_t s = 1; s <= 6; ++s) {
    if (active) ntt_sub_stage(buf, 6, s, W, (flags & NTT_INV) != 0, lane, 64);
    __syncthreads();
  }
  if (active) ntt_p2_store(buf, dst + b * dst_stride, logn, flags, k1, lane, 64);
}

// Workgroup (b, p): cell p of blob b's n_present cells, lane j its element j, to ext[b][64 idx[p] + j] (ext is
// zeroed before: the missing cells).  bad[b] (zeroed before) becomes 1 if an element is not below r.
__global__ void __launch_bounds__(64) k_cells_scatter(const uint8_t* cells, const uint32_t* idx, uint32_t n_present,
                                                      Fr* ext, int* bad) {
  const size_t b = blockIdx.x / n_present;
  const uint32_t p = blockIdx.x % n_present, j = threadIdx.x;
  const uint32_t k = idx[p] & (NTT_CELLS - 1);
  Fr v;
  if (!fr_from_be32(v, cells + ((b * n_present + p) * NTT_CELL + j) * 32)) bad[b] = 1;
  ext[b * NTT_EXT + k * NTT_CELL + j] = v;
}

// present: 128 flags.  zd[m] = Z(w^m), zci[m] = 1 / Z(7 w^m), m < 128 (both repeat with period 128 over the domain)
__global__ void __launch_bounds__(128) k_cells_vanish(const uint8_t* present, const Fr* W, Fr* zd, Fr* zci) {
  __shared__ Fr coef[NTT_CELLS + 1];
  __shared__ uint32_t sh_deg;
  if (threadIdx.x == 0) sh_deg = cells_vanishing(present, W, coef);
  __syncthreads();
  const uint32_t m = threadIdx.x, deg = sh_deg;
  zd[m] = cells_vanish_domain(coef, deg, W, m);
  zci[m] = fr_inv(cells_vanish_coset(coef, deg, W, m));
}

// dst[b][i] = src[b][brp ? brp13(i) : i] mul[i & mask] for i < dst_n (src: 8,192 per blob)
__global__ void __launch_bounds__(256) k_cells_pointwise(const Fr* src, Fr* dst, uint32_t dst_n, size_t total,
                                                         uint32_t brp, const Fr* mul, uint32_t mask) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= total) return;
  const size_t b = g / dst_n;
  const uint32_t i = (uint32_t)(g % dst_n);
  dst[g] = cells_pointwise(src + b * NTT_EXT, i, brp != 0, mul, mask);
}

__global__ void __launch_bounds__(256) k_fr_encode(const Fr* in, size_t n, uint8_t* out32) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) fr_to_be32(in[i], out32 + 32 * i);
}

// ------------------------------------------------------------------------------------------------ verification --
// item = blockIdx.x * 4 + wave; lane j holds element j.  The cell in the spec's order is the sub-transform's
// bit-reversed input (bls_fr_ntt.h).  cok[item] = every element < r and the cell index < 128.
__global__ void __launch_bounds__(256) k_cells_interp(const uint8_t* cells, const uint32_t* kidx, size_t n, const Fr* W,
                                                      Fr* coef, int* cok) {
  __shared__ Fr sh[NTT_WAVES][NTT_CELL];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const size_t item = (size_t)blockIdx.x * NTT_WAVES + wave;
  const bool active = item < n;
  Fr* buf = sh[wave];
  uint32_t k = 0;
  int good = 1;
  if (active) {
    k = kidx[item];
    Fr v;
    good = fr_from_be32(v, cells + (item * NTT_CELL + lane) * 32) ? 1 : 0;
    buf[lane] = v;
  }
  __syncthreads();
#pragma unroll 1
  for (uint32_t s = 1; s <= 6; ++s) {
    if (active) ntt_sub_stage(buf, 6, s, W, true, lane, 64);
    __syncthreads();
  }
  if (!active) return;  // a whole wave
  cells_interp_scale(buf, k, W, lane, 64);  // lane m reads and writes entry m alone
  coef[item * NTT_CELL + lane] = buf[lane];
  const int all = __all(good);
  if (lane == 0) cok[item] = (all && k < NTT_CELLS) ? 1 : 0;
}

// Item k's r_k: the first 16 bytes of SHA-256(seed32 || k as 8 big-endian bytes), a 128-bit integer, as k_kzg_rlc
// derives it.  Points P (nc + 2 n + 1; the caller decoded the commitments into P[0 .. nc) and the proofs into
// P[nc .. nc + n)) and their scalar rows k32:
//   [0, nc)                   C_i     (k_cells_weights)
//   [nc, nc + n)              pi_k    r_k h_k^64
//   nc + n                    identity, scalar 0: k_cells_put stores the interpolants' sum over its product
//   [nc + n + 1, nc + 2 n + 1)  pi_k  r_k
// One workgroup; lanes stride over the items.
__global__ void __launch_bounds__(256) k_cells_rlc(const uint8_t* seed32, size_t nc, size_t n, const uint32_t* kidx,
                                                   const Fr* W, Fr* rfr, G1A* P, uint8_t* k32) {
#pragma unroll 1
  for (size_t i = threadIdx.x; i < n; i += 256) {
    Sha256 s;
    sha256_init(s);
    sha256_update(s, seed32, 32);
    for (int b = 7; b >= 0; --b) sha256_byte(s, (uint8_t)((uint64_t)i >> (8 * b)));
    uint8_t h[32];
    sha256_final(s, h);
    uint8_t rb[32];
    for (int b = 0; b < 16; ++b) rb[b] = 0, rb[16 + b] = h[b];
    const Fr r = fr_to_mont(fr_raw_from_be32(rb));  // < 2^128 < r
    rfr[i] = r;
    for (int b = 0; b < 32; ++b) k32[32 * (nc + n + 1 + i) + b] = rb[b];
    fr_to_be32(fr_mul(r, cells_shift_pow64(W, kidx[i])), k32 + 32 * (nc + i));
    P[nc + n + 1 + i] = P[nc + i];
  }
  if (threadIdx.x) return;
  for (int b = 0; b < 32; ++b) k32[32 * (nc + n) + b] = 0;
  P[nc + n] = G1A{fp_zero(), fp_zero(), true};
}

// lane i: commitment i's weight, the sum of r_k over the items that name it (n nc additions in all)
__global__ void __launch_bounds__(64) k_cells_weights(size_t nc, size_t n, const uint32_t* cidx, const Fr* rfr,
                                                      uint8_t* k32) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nc) return;
  Fr acc = fr_zero();
#pragma unroll 1
  for (size_t k = 0; k < n; ++k)
    if (cidx[k] == i) acc = fr_add(acc, rfr[k]);
  fr_to_be32(acc, k32 + 32 * i);
}

// level 1: workgroup g, lane m: part[g][m] = sum over cells k in [64 g, 64 g + 64) of r_k c_{k,m}
__global__ void __launch_bounds__(64) k_cells_colsum(const Fr* coef, const Fr* rfr, size_t n, Fr* part) {
  const uint32_t m = threadIdx.x;
  const size_t k0 = (size_t)blockIdx.x * NTT_CELL;
  const size_t k1 = k0 + NTT_CELL < n ? k0 + NTT_CELL : n;
  Fr acc = fr_zero();
#pragma unroll 1
  for (size_t k = k0; k < k1; ++k) acc = fr_add(acc, fr_mul(rfr[k], coef[k * NTT_CELL + m]));
  part[(size_t)blockIdx.x * NTT_CELL + m] = acc;
}
// level 2: lane m: row m = -sum_g part[g][m] (the table MSM then gives -sum_m s_m [tau^m]_1)
__global__ void __launch_bounds__(64) k_cells_colsum2(const Fr* part, size_t groups, uint8_t* k32) {
  const uint32_t m = threadIdx.x;
  Fr acc = fr_zero();
#pragma unroll 1
  for (size_t g = 0; g < groups; ++g) acc = fr_add(acc, part[g * NTT_CELL + m]);
  fr_to_be32(fr_neg(acc), k32 + 32 * m);
}

__global__ void k_cells_put(const G1A* aff, const int* aff_live, G1A* S, int* live) {
  if (threadIdx.x || blockIdx.x) return;
  *S = *aff;
  *live = *aff_live;
}

// item k's pairs (pi_k, -[tau^64] G2) and (C_k - I_k + [h_k^64] pi_k, G2) at P / Q[2 k], [2 k + 1]; CP: the decoded
// commitments (nc), then the proofs; I: the interpolants' commitments (rows of the table MSM)
__global__ void __launch_bounds__(64) k_cells_item_pairs(size_t nc, size_t n, const G1A* CP, const uint32_t* cidx,
                                                         const uint32_t* kidx, const G1A* I, const Fr* W,
                                                         const G2A* negtau64, G1A* P, G2A* Q) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const G1A pi = CP[nc + i];
  const uint32_t c = cidx[i] < nc ? cidx[i] : 0;
  const Fr h = fr_from_mont(cells_shift_pow64(W, kidx[i]));
  G1J x = jac_from_aff(CP[c]);
  x = jac_add(x, jac_neg(jac_from_aff(I[i])));
  x = jac_add(x, jac_mul_u256(jac_from_aff(pi), h.l));
  P[2 * i] = pi;
  Q[2 * i] = *negtau64;
  P[2 * i + 1] = jac_to_aff(x);
  Q[2 * i + 1] = g2_generator();
}

// ======================================================= host launchers ==
#define LAUNCH(k, g, b, st, ...)                                 \
  do {                                                           \
    hipLaunchKernelGGL(k, dim3(g), dim3(b), 0, st, __VA_ARGS__); \
    hipError_t e__ = hipGetLastError();                          \
    if (e__ != hipSuccess) return e__;                           \
  } while (0)

size_t ntt_tables_bytes() { return 3 * (size_t)NTT_EXT * sizeof(Fr); }

hipError_t launch_ntt_tables(hipStream_t st, Fr* tab) {
  LAUNCH(k_ntt_tables, 3 * NTT_EXT / 256, 256, st, tab);
  return hipSuccess;
}

hipError_t launch_ntt(hipStream_t st, const Fr* W, uint32_t logn, uint32_t flags, uint32_t limit, size_t B,
                      const Fr* src, size_t src_stride, Fr* tmp, Fr* dst, size_t dst_stride) {
  if (!B) return hipSuccess;
  if (logn != 12 && logn != 13) return hipErrorInvalidValue;
  const uint32_t t1 = (uint32_t)B * 64, t2 = (uint32_t)B << (logn - 6);
  LAUNCH(k_ntt_pass1, nblk(t1, NTT_WAVES), NTT_WG, st, src, src_stride, tmp, W, logn, flags, limit, t1);
  LAUNCH(k_ntt_pass2, nblk(t2, NTT_WAVES), NTT_WG, st, tmp, dst, dst_stride, W, logn, flags, t2);
  return hipSuccess;
}

hipError_t launch_cells_scatter(hipStream_t st, const uint8_t* cells, const uint32_t* idx, uint32_t n_present, size_t B,
                                Fr* ext, int* bad) {
  if (!B || !n_present) return hipSuccess;
  LAUNCH(k_cells_scatter, (unsigned)(B * n_present), NTT_CELL, st, cells, idx, n_present, ext, bad);
  return hipSuccess;
}

hipError_t launch_cells_vanish(hipStream_t st, const uint8_t* present, const Fr* W, Fr* zd, Fr* zci) {
  LAUNCH(k_cells_vanish, 1, NTT_CELLS, st, present, W, zd, zci);
  return hipSuccess;
}

hipError_t launch_cells_pointwise(hipStream_t st, const Fr* src, Fr* dst, uint32_t dst_n, size_t B, bool brp,
                                  const Fr* mul, uint32_t mask) {
  if (!B) return hipSuccess;
  const size_t total = B * dst_n;
  LAUNCH(k_cells_pointwise, nblk(total, 256), 256, st, src, dst, dst_n, total, brp ? 1u : 0u, mul, mask);
  return hipSuccess;
}

hipError_t launch_fr_encode(hipStream_t st, const Fr* in, size_t n, uint8_t* out32) {
  if (!n) return hipSuccess;
  LAUNCH(k_fr_encode, nblk(n, 256), 256, st, in, n, out32);
  return hipSuccess;
}


hipError_t launch_cells_interp(hipStream_t st, const uint8_t* cells, const uint32_t* kidx, size_t n, const Fr* W,
                               Fr* coef, int* cok) {
  if (!n) return hipSuccess;
  LAUNCH(k_cells_interp, nblk(n, NTT_WAVES), NTT_WG, st, cells, kidx, n, W, coef, cok);
  return hipSuccess;
}

size_t cells_colsum_groups(size_t n) { return (n + NTT_CELL - 1) / NTT_CELL; }

hipError_t launch_cells_rlc(hipStream_t st, const uint8_t* seed32, size_t nc, size_t n, const uint32_t* cidx,
                            const uint32_t* kidx, const Fr* W, const Fr* coef, Fr* rfr, Fr* part, G1A* P, uint8_t* k32,
                            uint8_t* rli32) {
  LAUNCH(k_cells_rlc, 1, 256, st, seed32, nc, n, kidx, W, rfr, P, k32);
  LAUNCH(k_cells_weights, nblk(nc, 64), 64, st, nc, n, cidx, rfr, k32);
  const size_t groups = cells_colsum_groups(n);
  LAUNCH(k_cells_colsum, (unsigned)groups, NTT_CELL, st, coef, rfr, n, part);
  LAUNCH(k_cells_colsum2, 1, NTT_CELL, st, part, groups, rli32);
  return hipSuccess;
}

hipError_t launch_cells_put(hipStream_t st, const G1A* aff, const int* aff_live, G1A* S, int* live) {
  LAUNCH(k_cells_put, 1, 64, st, aff, aff_live, S, live);
  return hipSuccess;
}

hipError_t launch_cells_item_pairs(hipStream_t st, size_t nc, size_t n, const G1A* CP, const uint32_t* cidx,
                                   const uint32_t* kidx, const G1A* I, const Fr* W, const G2A* negtau64, G1A* P,
                                   G2A* Q) {
  if (!n) return hipSuccess;
  LAUNCH(k_cells_item_pairs, nblk(n, 64), 64, st, nc, n, CP, cidx, kidx, I, W, negtau64, P, Q);
  return hipSuccess;
}

}  // namespace bls
