// Where the KeyValidate kernels leave a key's result (k_key_validate: one key per lane, bls_kernels.hip;
// k_key_validate_wide: two keys per four-wave workgroup, bls_wide.hip).  The policy is the kernels' last argument
// and put() their only store: the arithmetic is the same instantiation-independent code, so a new destination costs
// a store sequence, never a copy of the chains.
//   put(i, a, ok): key i decoded to the affine point a (the identity when it failed) with verdict ok.
#pragma once
#include <cstddef>

#include "bls_ops.h"

namespace bls {

// the decoded point and its verdict in two arrays (the per-call paths; registry loads, which pack them afterwards)
struct KeyOutPoints {
  G1A* out;
  int* ok;
  __device__ __forceinline__ void put(size_t i, const G1A& a, int v) const {
    out[i] = a;
    ok[i] = v;
  }
};

// a RegKey record as the registry stores it (k_reg_pack): (x, y), the verdict in REG_VALID, a failed key all zero --
// the key table of a keys batch (bls_fav_batch_keys), written straight from the key bytes; valid (nullable): the
// verdict as a byte for the host
static_assert(sizeof(RegKey) == 128 && offsetof(RegKey, y) == 48 && offsetof(RegKey, pad) == 96,
              "KeyOutRecords::put stores a record as x | y | pad in eight 16-byte pieces");
struct KeyOutRecords {
  RegKey* rec;
  uint8_t* valid;
  __device__ __forceinline__ void put(size_t i, const G1A& a, int v) const {
    // eight 16-byte stores from the registers the point is in -- x, y (a failed key zeroed, the verdict OR-ed into
    // x's top word), then literal zeros for the pad: no RegKey temporary, which cost a private (or LDS) copy of the pad
    uint4* r = reinterpret_cast<uint4*>(rec + i);
    const uint32_t m = v ? 0xffffffffu : 0u;
#pragma unroll
    for (int w = 0; w < 3; ++w) {
      r[w] = make_uint4(a.x.l[4 * w] & m, a.x.l[4 * w + 1] & m, a.x.l[4 * w + 2] & m,
                        (a.x.l[4 * w + 3] & m) | (w == 2 ? (REG_VALID & m) : 0u));
      r[3 + w] = make_uint4(a.y.l[4 * w] & m, a.y.l[4 * w + 1] & m, a.y.l[4 * w + 2] & m, a.y.l[4 * w + 3] & m);
    }
    r[6] = make_uint4(0u, 0u, 0u, 0u);
    r[7] = make_uint4(0u, 0u, 0u, 0u);
    if (valid) valid[i] = v ? 1 : 0;
  }
};

}  // namespace bls
