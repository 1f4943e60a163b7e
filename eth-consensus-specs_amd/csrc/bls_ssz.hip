// SHA-256 node hashing for signing roots and SSZ merkleization (SURVEY.md
// §8(f) item 3): the step right before the verify path.
//   compute_signing_root(obj, domain) = hash_tree_root(SigningData(obj_root, domain))
//                                     = SHA-256(obj_root || domain)
//   (specs/phase0/beacon-chain.md:953-962, SigningData :317-320)
//   merkleize(chunks, limit): pairwise SHA-256 up a tree padded with zero
//   chunks to the next power of two (ssz/simple-serialize.md, "merkleize").
// One lane per 64-byte node: two compressions, the second a constant padding
// block (message length 512 bits).
#include "bls_kernels.h"
#include "bls_sha256.h"

namespace bls {

// SHA-256 of the 64-byte node in blk (sixteen big-endian words, clobbered): st = the digest's eight words
__device__ __forceinline__ void node_words(uint32_t* st, uint32_t* blk) {
#pragma unroll
  for (int k = 0; k < 8; k++) st[k] = SHA256_IV[k];
  sha256_compress(st, blk);
#pragma unroll
  for (int k = 0; k < 16; k++) blk[k] = 0;
  blk[0] = 0x80000000u;
  blk[15] = 512;
  sha256_compress(st, blk);
}

__device__ __forceinline__ uint32_t be32(const uint8_t* p) {
  return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
}

__device__ __forceinline__ void put_digest(uint8_t* out, const uint32_t* st) {
#pragma unroll
  for (int k = 0; k < 8; k++) {
    out[4 * k] = (uint8_t)(st[k] >> 24);
    out[4 * k + 1] = (uint8_t)(st[k] >> 16);
    out[4 * k + 2] = (uint8_t)(st[k] >> 8);
    out[4 * k + 3] = (uint8_t)st[k];
  }
}

__device__ __forceinline__ void node_hash(const uint8_t* l, const uint8_t* r, uint8_t* out) {
  uint32_t blk[16];
#pragma unroll
  for (int k = 0; k < 8; k++) {
    blk[k] = be32(l + 4 * k);
    blk[8 + k] = be32(r + 4 * k);
  }
  uint32_t st[8];
  node_words(st, blk);
  put_digest(out, st);
}

// out[i] = SHA-256(left[32 i ..] || right[rstride i ..])  (rstride 0: one shared right half, e.g. a domain)
__global__ void __launch_bounds__(64) k_sha256_pairs(const uint8_t* left, const uint8_t* right, size_t rstride,
                                                     size_t n, uint8_t* out) {
  const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (i < n) node_hash(left + 32 * i, right + rstride * i, out + 32 * i);
}

// one tree level: out[j] = H(in[2j] || in[2j+1]), the missing right sibling of an odd tail = zero[0]
__global__ void __launch_bounds__(64) k_merkle_level(const uint8_t* in, size_t n_in, const uint8_t* zero,
                                                     uint8_t* out) {
  const size_t j = (size_t)blockIdx.x * 64 + threadIdx.x;
  const size_t n_out = (n_in + 1) / 2;
  if (j >= n_out) return;
  const uint8_t* r = 2 * j + 1 < n_in ? in + 32 * (2 * j + 1) : zero;
  node_hash(in + 64 * j, r, out + 32 * j);
}

// zero[0] <- H(zero[0] || zero[0]): the zero-subtree root one level up
__global__ void k_zero_up(uint8_t* zero) {
  if (threadIdx.x || blockIdx.x) return;
  uint8_t t[32];
  node_hash(zero, zero, t);
  for (int k = 0; k < 32; k++) zero[k] = t[k];
}

// Deposit signing roots (is_valid_deposit_signature, specs/electra/beacon-chain.md:1577-1588): one lane per deposit,
//   out[i] = compute_signing_root(DepositMessage(pubkey_i, withdrawal_credentials_i, amount_i), domain)
// as five 64-byte nodes -- the container has three fields, so four leaves:
//   k = H(pk[0:32] || pk[32:48] 0^16)      hash_tree_root(Bytes48)
//   a = H(k || wc)    b = H(le64(amount) 0^24 || 0^32)    root = H(a || b)    out = H(root || domain)
// The digests stay in registers as words between the nodes; only the inputs and the result touch memory.
__global__ void __launch_bounds__(64) k_deposit_roots(const uint8_t* pks48, const uint8_t* wc32,
                                                      const uint64_t* amounts, const uint8_t* domain32, size_t n,
                                                      uint8_t* out32) {
  const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  uint32_t blk[16], a[8], b[8];
#pragma unroll
  for (int k = 0; k < 12; k++) blk[k] = be32(pks48 + 48 * i + 4 * k);
#pragma unroll
  for (int k = 12; k < 16; k++) blk[k] = 0;
  node_words(a, blk);
#pragma unroll
  for (int k = 0; k < 8; k++) {
    blk[k] = a[k];
    blk[8 + k] = be32(wc32 + 32 * i + 4 * k);
  }
  node_words(a, blk);
  const uint64_t amt = amounts[i];
#pragma unroll
  for (int k = 0; k < 16; k++) blk[k] = 0;
  blk[0] = __builtin_bswap32((uint32_t)amt);  // the little-endian bytes of the amount, read as big-endian words
  blk[1] = __builtin_bswap32((uint32_t)(amt >> 32));
  node_words(b, blk);
#pragma unroll
  for (int k = 0; k < 8; k++) {
    blk[k] = a[k];
    blk[8 + k] = b[k];
  }
  node_words(a, blk);
#pragma unroll
  for (int k = 0; k < 8; k++) {
    blk[k] = a[k];
    blk[8 + k] = be32(domain32 + 4 * k);
  }
  node_words(a, blk);
  put_digest(out32 + 32 * i, a);
}

hipError_t launch_deposit_roots(hipStream_t st, const uint8_t* pks48, const uint8_t* wc32, const uint64_t* amounts,
                                const uint8_t* domain32, size_t n, uint8_t* out32) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(k_deposit_roots, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, pks48, wc32, amounts, domain32,
                     n, out32);
  return hipGetLastError();
}

hipError_t launch_sha256_pairs(hipStream_t st, const uint8_t* left, const uint8_t* right, size_t rstride, size_t n,
                               uint8_t* out) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(k_sha256_pairs, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, left, right, rstride, n, out);
  return hipGetLastError();
}

// depth levels over n >= 1 chunks in a (ping-pong with b); zero: 32 zeroed device bytes (clobbered).
// Returns the buffer holding the root.
hipError_t launch_merkleize(hipStream_t st, uint8_t* a, uint8_t* b, size_t n, int depth, uint8_t* zero,
                            uint8_t** root) {
  uint8_t *cur = a, *nxt = b;
  for (int l = 0; l < depth; l++) {
    hipLaunchKernelGGL(k_merkle_level, dim3((unsigned)(((n + 1) / 2 + 63) / 64)), dim3(64), 0, st, cur, n, zero, nxt);
    hipLaunchKernelGGL(k_zero_up, dim3(1), dim3(64), 0, st, zero);
    n = (n + 1) / 2;
    uint8_t* t = cur;
    cur = nxt;
    nxt = t;
  }
  *root = cur;
  return hipGetLastError();
}

}  // namespace bls
