// Committee-bitfield FAV items (bls_fav_batch_committee_bits): an item names committees of a device-resident table
// and carries one participation bit per member, as an attestation does (get_attesting_indices).  Its aggregate key
// is either the sum of the participants' keys (direct) or, when that adds fewer points, the committees' cached sums
// minus the non-participants' keys (complement, as process_sync_aggregate does for the sync committee):
//   direct      p additions                          p = bits set, n = members of the item's committees
//   complement  (n - p) + ncomm additions            ncomm = committees of the item
// A wave expands each item into the list of registry indices the gather adds (bits_expand_item), and each gather
// lane of a complement item turns its partial sum S_l into base_l - S_l, base_l its strided share of the committee
// sums (bits_lane_combine): sum_l (base_l - S_l) = base - S, so the gather's own tree finishes both forms.
//
// Everything here is the code the kernels (bls_gather_bits.hip) and the host check (tests/hostcheck_bits, with
// BLS_FQ_CHECK) both run; the wave-wide steps go through an executor (ballot / sum / all / each over 64 lanes) that
// the kernel maps to the wave's cross-lane operations and the host check to loops.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "bls_curve.h"
#include "bls_fq_g1.h"

namespace bls {

constexpr int BITS_MODE_AUTO = 0, BITS_MODE_DIRECT = 1, BITS_MODE_COMPLEMENT = 2;
// BitsItem::flags
constexpr uint32_t BITS_F_COMPLEMENT = 1;  // the list holds the non-participants: aggregate = committee sums - list
constexpr uint32_t BITS_F_MALFORMED = 2;   // a padding bit of the last byte is set: verdict 0
constexpr uint32_t BITS_F_SOME = 4;        // at least one bit set (FastAggregateVerify of no key is false)

// One item's list for the gather: registry indices list[start .. start + len).  start is the prefix sum of the
// items' member counts, so the host knows it without reading anything back.
struct BitsItem {
  uint64_t start;
  uint32_t len, flags;
};

// bit k of an SSZ bitfield without its delimiter
BLS_HD uint32_t bits_get(const uint8_t* bits, uint64_t k) { return (bits[k >> 3] >> (k & 7)) & 1u; }

// a bit at a position >= n of the last byte
BLS_HD bool bits_padding_set(const uint8_t* bits, uint64_t n) { return (n & 7) && (bits[n >> 3] >> (n & 7)) != 0; }

// The form counts point additions, so it is not a tuning knob: complement iff it adds fewer.  It needs every
// committee's cached sum to be usable (all_cstat: every member in range and valid when the table was loaded) --
// otherwise a bad NON-participant, which FastAggregateVerify never looks at, would spoil the item.
BLS_HD bool bits_use_complement(int mode, uint64_t n, uint64_t p, uint64_t ncomm, bool all_cstat) {
  if (!all_cstat || mode == BITS_MODE_DIRECT) return false;
  if (mode == BITS_MODE_COMPLEMENT) return true;
  return (n - p) + ncomm < p;
}

// An item with no bit set or a padding bit set has verdict 0 whatever its keys are: its list is empty.
BLS_HD BitsItem bits_item_header(int mode, uint64_t start, uint64_t n, uint64_t p, uint64_t ncomm, bool all_cstat,
                                 bool malformed) {
  BitsItem it{start, 0, malformed ? BITS_F_MALFORMED : 0u};
  if (malformed || p == 0) return it;
  it.flags = BITS_F_SOME;
  if (bits_use_complement(mode, n, p, ncomm, all_cstat)) {
    it.flags |= BITS_F_COMPLEMENT;
    it.len = (uint32_t)(n - p);
  } else {
    it.len = (uint32_t)p;
  }
  return it;
}

// the list slot of lane `lane` among the wanted lanes `mask` of a 64-position step, after cnt earlier entries
BLS_HD uint64_t bits_slot(uint64_t cnt, uint64_t mask, uint32_t lane) {
  return cnt + (uint64_t)__builtin_popcountll(mask & ((1ull << lane) - 1));
}

// One item on one wave.  comm_ids[0 .. ncomm): its committees, tab_idx / tab_offs / cstat: the table; bits: its
// ceil(n / 8) bytes, n its member count.  Writes the wanted members' registry indices -- bit 1 for direct, bit 0 for
// complement, in member order -- to list[start ..) and returns the item's record.  Every variable outside the
// executor's callbacks is wave-uniform.
template <class Ex>
BLS_HD BitsItem bits_expand_item(Ex& ex, int mode, const uint32_t* __restrict__ comm_ids, uint64_t ncomm,
                                 const uint32_t* __restrict__ tab_idx, const uint64_t* __restrict__ tab_offs,
                                 const int* __restrict__ cstat, const uint8_t* __restrict__ bits, uint64_t n,
                                 uint64_t start, uint32_t* __restrict__ list) {
  const uint64_t nbytes = (n + 7) / 8;
  const uint64_t p = ex.sum([&](uint32_t l) {
    uint64_t s = 0;
    for (uint64_t i = l; i < nbytes; i += 64) s += (uint64_t)__builtin_popcount(bits[i]);
    return s;
  });
  const bool all_cstat = ex.all([&](uint32_t l) {
    bool ok = true;
    for (uint64_t j = l; j < ncomm; j += 64) ok = ok && cstat[comm_ids[j]] != 0;
    return ok;
  });
  const BitsItem it = bits_item_header(mode, start, n, p, ncomm, all_cstat, bits_padding_set(bits, n));
  if (!it.len) return it;
  const uint32_t want = (it.flags & BITS_F_COMPLEMENT) ? 0u : 1u;
  uint64_t cnt = 0, pos0 = 0;
  for (uint64_t j = 0; j < ncomm; ++j) {
    const uint64_t lo = tab_offs[comm_ids[j]], size = tab_offs[comm_ids[j] + 1] - lo;
    for (uint64_t m0 = 0; m0 < size; m0 += 64) {
      const uint64_t mask =
          ex.ballot([&](uint32_t l) { return m0 + l < size && bits_get(bits, pos0 + m0 + l) == want; });
      ex.each([&](uint32_t l) {  // the member's index is read beside its bit, not after the ballot
        const uint32_t key = m0 + l < size ? tab_idx[lo + m0 + l] : 0u;
        if ((mask >> l) & 1) list[start + bits_slot(cnt, mask, l)] = key;
      });
      cnt += (uint64_t)__builtin_popcountll(mask);
    }
    pos0 += size;
  }
  return it;
}

// -(X : Y : Z) = (X : -Y : Z) of a gather accumulator -- the identity (0 : 1 : 0) in N form or an output of
// g1q_add_aff / g1q_add, so Y is inside the accumulator bound AccYZ (< 4p, digits <= 2^29 + 2^4).  -Y = K - Y
// digit-wise with K the smallest multiple of p whose borrowed digits cover AccYZ (bls_fqb.h neg), normalised; the
// relax to AccX compiles only if that value and those digits are inside what g1q_add takes for any operand
// coordinate (< 66p, digits <= 2^29 + 2^4), so the bound is proved here and not assumed.
BLS_HD G1Q g1q_neg_acc(const G1Q& a) {
  using namespace g1q_detail;
  const auto ny = norm(neg(AccYZ{a.y}));
  return G1Q{a.x, relax<AccX::val, AccX::dig>(ny).x, a.z};
}

// A gather lane's last step: S_l for a direct item; for a complement item base_l - S_l, base_l the sum of the
// item's committee sums j = lane, lane + L, ... (stored canonical: N form after fq_unpack, a g1q_add operand).
// g1q_add's outputs are N form, accumulators again, so the loop closes and the gather's tree takes the result.
BLS_HD G1Q bits_lane_combine(G1Q acc, uint32_t flags, const uint32_t* comm_ids, uint64_t ncomm, const G1P* csum,
                             uint32_t lane, uint32_t L) {
  if (!(flags & BITS_F_COMPLEMENT)) return acc;
  acc = g1q_neg_acc(acc);
#pragma unroll 1
  for (uint64_t j = lane; j < ncomm; j += L) {
    const G1P& s = csum[comm_ids[j]];
    acc = g1q_add(acc, G1Q{fq_unpack(s.x), fq_unpack(s.y), fq_unpack(s.z)});
  }
  return acc;
}

}  // namespace bls
