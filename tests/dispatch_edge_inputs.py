"""Inputs of the dispatch-edge tests (tests/test_gpu_sum_edges.py, tests/test_gpu_percall_thresholds.py) and of their
CPU self-check (tests/test_dispatch_edges_cpu.py): pure-Python constructions, nothing here touches the device.

Keys: pk_i = [i + 1] G1, so sk(i) = i + 1.  The negation of a compressed point is the same encoding with the sign
flag 0x20 flipped, and the secret of a negated key is r - (i + 1).  A layout is a list of (key index, negated?), one
entry per position of the key list a call receives; expected_sum(layout) is the sum of the secrets mod r, so every
expected G1 sum is one SkToPk(s) -- and the identity for s = 0, where the tests ask the oracle what it does with the
same bytes.

Where the members of a layout land:
  k_g1_sum_q (n <= G1Q_SUM_MAX, one workgroup):  position p -> lane p % 256; the lane adds its positions in order
      (g1q_add_aff), then the LDS tree adds lane t + s into lane t for s = 128, 64, .., 1 (g1q_add).
  k_g1_sum_aff<64> + k_jac_sum (above), k_g2_sum_aff, k_pt_sum + k_pt_sum_jac (every n): position p -> block
      p // 64, lane p % 64 while there are at most 1,024 blocks (one point per lane; beyond, block b also takes
      positions p + 65,536 j); the block's tree adds lane t + s into lane t for s = 32, .., 1; the second kernel
      gives partial b to lane b % 64 and runs the same tree."""
from oracle import bls_oracle as O

R = O.R
G1_INF = b"\xc0" + bytes(47)
G2_INF = b"\xc0" + bytes(95)

# ---- the thresholds as the tests use them, each with the source line it mirrors (test_dispatch_edges_cpu.py checks
# the text of those files against SOURCE_CONSTANTS below) ----
G1Q_SUM_NT = 256               # csrc/bls_kernels.hip:101  constexpr int G1Q_SUM_NT = 256;
G1Q_SUM_MAX = 8 * G1Q_SUM_NT   # csrc/bls_kernels.hip:102  constexpr size_t G1Q_SUM_MAX = 8 * G1Q_SUM_NT;  (:529 n <=)
SUM_BLOCK = 64                 # csrc/bls_kernels.hip:533,541 nblk(n, 64); csrc/bls_points.hip:190 pblk
SUM_MAX_BLOCKS = 1024          # csrc/bls_kernels.hip:534,542; csrc/bls_points.hip:217  if (g > 1024) g = 1024;
WIDE_KEYS_MAX = 4096           # csrc/bls_capi_ctx.hip:79  constexpr size_t WIDE_KEYS_MAX = 4096;
WIDE_H2C_MAX = 1024            # csrc/bls_capi_ctx.hip:18  env_long("BLS_WIDE_H2C_MAX", 1024)
WIDE_MILLER_MAX = 1100         # csrc/bls_capi_ctx.hip:19  env_long("BLS_WIDE_MILLER_MAX", 1100)
AVB_FUSED_MIN_NPAIR = 256      # csrc/bls_capi_percall.hip:446  if (npair >= 256)
MLF_PAIRS = 2                  # csrc/bls_wide.hip:702  constexpr int MLF_PAIRS = 2;

# the sizes the GPU tests straddle each switch with
G1_SUM_SIZES = (1, 2, 255, 256, 257, 513, 2047, 2048, 2049, 2113)
DEGENERATE_TOTALS = (G1Q_SUM_MAX, G1Q_SUM_MAX + 1)
KEY_SIZES = (WIDE_KEYS_MAX, WIDE_KEYS_MAX + 1)
AV_SIZES_32 = (1023, 1024, 1025, 1099, 1100, 1101)
AV_SIZES_MIXED = (1024, 1025, 1100)
MULTI_PAIRING_SIZES = (1, 2, 3, 1099, 1100)
MIXED_LENGTHS = (0, 1, 31, 32, 33, 100, 200)

# (constant name, file under eth-consensus-specs_amd/, pattern the file must still contain, the size lists above that
# have to move with it)
SOURCE_CONSTANTS = (
    ("G1Q_SUM_NT", "csrc/bls_kernels.hip", r"constexpr int G1Q_SUM_NT = %d;" % G1Q_SUM_NT,
     "the lane count of the layouts (layouts(total, lanes))"),
    ("G1Q_SUM_MAX", "csrc/bls_kernels.hip", r"constexpr size_t G1Q_SUM_MAX = 8 \* G1Q_SUM_NT;",
     "G1_SUM_SIZES, DEGENERATE_TOTALS"),
    ("G1Q_SUM_MAX", "csrc/bls_kernels.hip", r"if \(n <= G1Q_SUM_MAX\) \{", "G1_SUM_SIZES, DEGENERATE_TOTALS"),
    ("WIDE_KEYS_MAX", "csrc/bls_capi_ctx.hip", r"constexpr size_t WIDE_KEYS_MAX = %d;" % WIDE_KEYS_MAX, "KEY_SIZES"),
    ("WIDE_KEYS_MAX", "csrc/bls_capi_ctx.hip", r"return n <= WIDE_KEYS_MAX \? launch_key_validate_wide", "KEY_SIZES"),
    ("WIDE_KEYS_MAX", "csrc/bls_capi_ctx.hip", r"if \(subgroup && n <= WIDE_KEYS_MAX\)", "KEY_SIZES"),
    ("WIDE_H2C_MAX", "csrc/bls_capi_ctx.hip", r'env_long\("BLS_WIDE_H2C_MAX", %d\)' % WIDE_H2C_MAX,
     "AV_SIZES_32, AV_SIZES_MIXED"),
    ("WIDE_H2C_MAX", "csrc/bls_capi_percall.hip", r"if \(n <= wide_h2c_max\)", "AV_SIZES_32, AV_SIZES_MIXED"),
    ("WIDE_MILLER_MAX", "csrc/bls_capi_ctx.hip", r'env_long\("BLS_WIDE_MILLER_MAX", %d\)' % WIDE_MILLER_MAX,
     "AV_SIZES_32, AV_SIZES_MIXED, MULTI_PAIRING_SIZES"),
    ("WIDE_MILLER_MAX", "csrc/bls_capi_ctx.hip", r"if \(n <= knobs\(\)\.wide_miller_max\)",
     "AV_SIZES_32, AV_SIZES_MIXED, MULTI_PAIRING_SIZES"),
    ("AVB_FUSED_MIN_NPAIR", "csrc/bls_capi_percall.hip", r"if \(npair >= %d\)" % AVB_FUSED_MIN_NPAIR,
     "the item shapes of test_aggregate_verify_batch_across_256_pairs"),
    ("MLF_PAIRS", "csrc/bls_wide.hip", r"constexpr int MLF_PAIRS = %d;" % MLF_PAIRS,
     "the parity of AV_SIZES_32 (the tail workgroup of k_miller_wide)"),
    ("SUM_BLOCK", "csrc/bls_kernels.hip", r"unsigned g = nblk\(n, %d\);\n  if \(g > %d\) g = %d;"
     % (SUM_BLOCK, SUM_MAX_BLOCKS, SUM_MAX_BLOCKS), "the G2 / multi_exp sizes 63, 64, 65, 129 and 65,537"),
    ("SUM_BLOCK", "csrc/bls_points.hip", r"unsigned g = pblk\(n\);\n  if \(g > %d\) g = %d;"
     % (SUM_MAX_BLOCKS, SUM_MAX_BLOCKS), "the G2 / multi_exp sizes 63, 64, 65, 129 and 65,537"),
)


def sk(i: int) -> int:
    return i + 1


def neg(enc: bytes) -> bytes:
    """-P of a compressed G1 or G2 point: the other y (the identity has none and is left alone)"""
    return enc if enc[0] & 0x40 else bytes([enc[0] ^ 0x20]) + enc[1:]


def secret(index: int, negated: bool) -> int:
    return R - sk(index) if negated else sk(index)


def expected_sum(positions) -> int:
    return sum(secret(i, n) for i, n in positions) % R


def key_bytes(keys48: bytes, positions) -> list:
    """the compressed keys of a layout, from the table of pk_0, pk_1, .."""
    out = []
    for i, n in positions:
        k = keys48[48 * i: 48 * i + 48]
        out.append(neg(k) if n else k)
    return out


def plain(total: int) -> list:
    """position p holds key p"""
    return [(p, False) for p in range(total)]


def _repeat(total: int, a: int, b: int) -> list:
    assert 0 <= a < b < total
    lay = plain(total)
    lay[b] = (a, False)
    return lay


def _cancel(total: int, a: int, b: int) -> list:
    assert 0 <= a < b < total
    lay = plain(total)
    lay[b] = (a, True)
    return lay


def cancel_blocked(total: int) -> list:
    """keys 0 .. h - 1, then their negations in the same order (h = total // 2), then for an odd total key h.
    h = 1,024 and 256 lanes: position p and p + 1,024 share lane p % 256, so every lane's own sum is the identity,
    the tree adds identities only and k_g1_sum_q leaves through Z == 0; with total = 2,049 key 1,024 at position
    2,048 (lane 0) is the whole sum.  64-lane blocks: at 2,049 block b + 16 holds the negations of block b < 16 and
    k_jac_sum adds partial b + 16 = -partial b at its tree level s = 16.  At 2,050 (h = 1,025) the negations sit one
    lane further on, the partials of k_jac_sum are [4,096 b + 2,080] G1 for b < 16, [1,025 - 2,016] G1 for b = 16,
    -[4,096 c + 2,016] G1 for b = 16 + c and -[2,049] G1 for b = 32: after s = 32 and s = 16 lanes 1 .. 15 all hold
    [64] G1, so s = 8, 4, 2 are jac_add doublings (lane 1: 128, 256, 512; lane 0: -896, -768, -512) and s = 1 adds
    [512] G1 and its negation: the identity, next to the identity returns for the idle lanes 33 .. 63."""
    h = total // 2
    return [(i, False) for i in range(h)] + [(i, True) for i in range(h)] + ([(h, False)] if total % 2 else [])


def cancel_interleaved(total: int) -> list:
    """k, -k, k + 1, -(k + 1), ..: a key and its negation in neighbouring lanes 2k % lanes and 2k % lanes + 1, no lane
    cancels by itself, every pair meets in the last level of the tree; an odd total ends in one more key"""
    h = total // 2
    return [(i, n) for i in range(h) for n in (False, True)] + ([(h, False)] if total % 2 else [])


def equal_blocks(total: int, period: int = 32) -> list:
    """position p holds key p % period: lanes `period` apart (and, for 64-lane blocks, all blocks) hold equal sums,
    so the trees add P + P: the doubling branch of g1q_add and jac_add"""
    return [(p % period, False) for p in range(total)]


def layouts(total: int, lanes: int = G1Q_SUM_NT) -> dict:
    """The named degenerate layouts at `total` keys for a sum kernel of `lanes` lanes (256: k_g1_sum_q; the 64-lane
    blocks of the two-pass kernels see the same positions as block p // 64, lane p % 64).  j is a position with
    room for every partner below."""
    j = 3 % lanes
    half, eighth = max(lanes // 2, 1), max(lanes // 8, 1)
    assert total >= 2 * lanes and j + lanes < total
    return {
        # positions j and j + lanes: the same lane of k_g1_sum_q, P + P in its g1q_add_aff; blocks j // 64 and
        # (j + lanes) // 64 of the two-pass kernels, the equal partials' sums meet in k_jac_sum (jac_add)
        "repeat_same_lane": _repeat(total, j, j + lanes),
        # lanes 3 and 4: lane 3 folds into lane 1 (s = 2), lane 4 into lane 0 (s = 4), and the two sums that hold P
        # meet at the last tree level (s = 1) of either kernel
        "repeat_neighbours": _repeat(total, j, j + 1),
        # lanes j and j + lanes / 2: the first tree level of k_g1_sum_q (s = 128); blocks 0 and 2 above 2,048
        "repeat_half": _repeat(total, j, j + half),
        # lanes j and j + lanes / 8 (32): the first tree level (s = 32) of the 64-lane kernels
        "repeat_eighth": _repeat(total, j, j + eighth),
        # P at j, -P at j + lanes, the lane's further positions j + 2 lanes, .. after them: the accumulator of
        # k_g1_sum_q passes through the identity and goes on
        "cancel_same_lane": _cancel(total, j, j + lanes),
        # P and -P in lanes j, j + 1
        "cancel_neighbours": _cancel(total, j, j + 1),
        "cancel_blocked": cancel_blocked(total),
        "cancel_interleaved": cancel_interleaved(total),
    }


def non_subgroup_g1():
    """A point of E1(Fp) outside G1 (the cofactor is not 1): the first x >= 1 with x^3 + 4 a square."""
    x = 1
    while True:
        y = O.fp_sqrt((x ** 3 + 4) % O.P)
        if y is not None:
            pt = (x, y)
            if not O.g1_in_subgroup(pt):
                return pt
        x += 1


def bad_keys() -> dict:
    """the invalid keys of the KeyValidate switch tests"""
    return {
        "non_subgroup": O.g1_compress(non_subgroup_g1()),
        "identity": G1_INF,
        "flag_0x40": b"\x40" + bytes(47),
        "x_is_p": ((1 << 383) | O.P).to_bytes(48, "big"),  # the compression flag on x = p (not reduced)
    }


def mixed_messages(n: int) -> list:
    """n distinct messages whose lengths cycle through MIXED_LENGTHS"""
    out = []
    for i in range(n):
        ln = MIXED_LENGTHS[i % len(MIXED_LENGTHS)]
        body = b"".join(((i * 131 + k) & 0xFFFFFFFF).to_bytes(4, "little") for k in range((ln + 3) // 4))[:ln]
        out.append(body)
    return out
