// TEST HARNESS ONLY: host build of the committee-bitfield logic (bls_g1_bits.h: the item expansion that
// k_bits_expand runs on a wave and the lane combine base - S of k_fav_gather_bits) with the digit form's 128-bit
// column, value and subtraction-precondition checks compiled in (BLS_FQ_CHECK), for tests/test_committee_bits_cpu.py.
#define BLS_FQ_CHECK 1
#define BLS_HD __host__ __device__ inline  // no forced inlining in this (host-only, checked) unit
#include "bls_ops.h"
#include "bls_g1_bits.h"
#include <string.h>
#include <vector>
using namespace bls;

static Fp in_fp(const uint8_t* b) { return fp_to_mont(raw_from_be48(b)); }
static void out_fp(uint8_t* b, const Fp& a) { raw_to_be48(fp_from_mont(a), b); }

// the wave's executor as loops over 64 lanes
struct HostExec {
  template <class F>
  uint64_t ballot(F f) {
    uint64_t m = 0;
    for (uint32_t l = 0; l < 64; ++l)
      if (f(l)) m |= 1ull << l;
    return m;
  }
  template <class F>
  void each(F f) {
    for (uint32_t l = 0; l < 64; ++l) f(l);
  }
  template <class F>
  uint64_t sum(F f) {
    uint64_t s = 0;
    for (uint32_t l = 0; l < 64; ++l) s += f(l);
    return s;
  }
  template <class F>
  bool all(F f) {
    bool a = true;
    for (uint32_t l = 0; l < 64; ++l) a = f(l) && a;
    return a;
  }
};

// One item: info = {len, flags}.  list has n + start entries, which the caller pre-fills to see what was written.
extern "C" void hc_bits_expand(int mode, const uint32_t* comm_ids, uint64_t ncomm, const uint32_t* tab_idx,
                               const uint64_t* tab_offs, const int* cstat, const uint8_t* bits, uint64_t n,
                               uint64_t start, uint32_t* list, uint32_t* info) {
  HostExec ex;
  const BitsItem it = bits_expand_item(ex, mode, comm_ids, ncomm, tab_idx, tab_offs, cstat, bits, n, start, list);
  info[0] = it.len;
  info[1] = it.flags;
  info[2] = it.start == start ? 1 : 0;
}

// The end of k_fav_gather_bits for one item on L lanes: acc holds the lanes' partial sums as raw digits (3 x 14 u32
// each, so the test picks their redundant form), csum the table's sums as canonical projective X || Y || Z (48 B
// big-endian each).  Every lane combines, the tree of complete additions follows; out = the affine result x || y,
// *inf = 1 for the identity.
extern "C" void hc_bits_combine(const uint32_t* acc, uint32_t L, uint32_t flags, const uint32_t* comm_ids,
                                uint64_t ncomm, const uint8_t* csum, size_t C, uint8_t* out, int* inf) {
  std::vector<G1P> cs(C);
  for (size_t c = 0; c < C; ++c)
    cs[c] = G1P{in_fp(csum + 144 * c), in_fp(csum + 144 * c + 48), in_fp(csum + 144 * c + 96)};
  std::vector<G1Q> sh(L);
  for (uint32_t l = 0; l < L; ++l) {
    G1Q a;
    memcpy(a.x.d, acc + 42 * l, 56);
    memcpy(a.y.d, acc + 42 * l + 14, 56);
    memcpy(a.z.d, acc + 42 * l + 28, 56);
    sh[l] = bits_lane_combine(a, flags, comm_ids, ncomm, cs.data(), l, L);
  }
  for (uint32_t s = L / 2; s > 0; s >>= 1)
    for (uint32_t l = 0; l < s; ++l) sh[l] = g1q_add(sh[l], sh[l + s]);
  const G1P o{fq_pack(sh[0].x), fq_pack(sh[0].y), fq_pack(sh[0].z)};
  memset(out, 0, 96);
  *inf = fp_is_zero(o.z) ? 1 : 0;
  if (*inf) return;
  const Fp zi = fp_inv(o.z);
  out_fp(out, fp_mul(o.x, zi));
  out_fp(out + 48, fp_mul(o.y, zi));
}
