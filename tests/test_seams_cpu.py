"""The batch-size seams the GPU tests cross (tests/seam_sizes.py) against the text of csrc/ and bls_mi355x/, and the
input builders of those tests against the oracle: rows_with_known_sums' spot rows against g1_mul, the linear items'
(y, proof) against KnownAnswer.open."""
import os
import random
import re

import g1_table_edge_inputs as E
import kzg_inputs as K
import seam_sizes as Z
from oracle import bls_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "eth-consensus-specs_amd")
R = O.R


def text(*path):
    with open(os.path.join(PKG, *path)) as fh:
        return fh.read()


def constant(src, pattern):
    m = re.search(pattern, src)
    assert m, pattern
    return int(m.group(1))


def test_seam_sizes_match_the_source():
    """Each constant is read where it is defined.  When one fails, the sizes tests/seam_sizes.py derives from it are
    the ones to move: SCAN_BLK / G1M_SLOTS / SCAN_TOP / FINAL_LANES -> MSM_ROWS*; G1Q_SUM_* -> KZG_VALID, KZG_FAILING,
    CELLS_VALID; RLC_LANES -> KZG_VALID, KZG_FAILING, KZG_BAD_AT and the distance of the offsetting-error tests;
    KZC_MSM_ROWS -> CELLS_FAILING, CELLS_BAD_AT; the *_MAX limits -> the refusal tests."""
    table = text("csrc", "bls_g1_table.hip")
    assert constant(table, r"constexpr uint32_t SCAN_BLK = (\d+);") == Z.SCAN_BLK
    assert constant(text("csrc", "bls_g1_msm.h"), r"constexpr uint32_t G1M_SLOTS = (\d+);") == Z.G1M_SLOTS
    assert Z.SCAN_BLK % Z.G1M_SLOTS == 0
    top = re.search(r"__launch_bounds__\((\d+)\) k_g1m_scan_top\(.*?\n}\n", table, re.S)
    assert top and int(top.group(1)) == Z.SCAN_TOP
    assert "r += %d)" % Z.SCAN_TOP in top.group(0) and "dim3(1), dim3(%d), 0, st, bsum, nb" % Z.SCAN_TOP in table
    for kernel in ("k_g1m_final", "k_g1m_compress"):
        m = re.search(r"__launch_bounds__\((\d+)\) %s\(.*?blockIdx\.x \* (\d+) \+ threadIdx\.x" % kernel, table, re.S)
        assert m and int(m.group(1)) == int(m.group(2)) == Z.FINAL_LANES, kernel
    assert constant(text("csrc", "bls_capi_msm.hip"), r"constexpr size_t G1M_BMAX = (\d+);") == Z.G1M_BMAX
    kern = text("csrc", "bls_kernels.hip")
    assert constant(kern, r"constexpr int G1Q_SUM_NT = (\d+);") == Z.G1Q_SUM_NT
    assert constant(kern, r"constexpr size_t G1Q_SUM_MAX = (\d+) \* G1Q_SUM_NT;") * Z.G1Q_SUM_NT == Z.G1Q_SUM_MAX
    assert "if (n <= G1Q_SUM_MAX) {" in kern
    assert constant(text("csrc", "bls_kzg_blob.h"), r"constexpr uint32_t KZB_LANES = (\d+);") == Z.RLC_LANES
    kzg = text("csrc", "bls_kzg.hip")
    assert "i < n; i += KZB_LANES)" in kzg and "LAUNCH(k_kzg_rlc, 1, KZB_LANES," in kzg
    cells = text("csrc", "bls_kzg_cells.hip")
    assert "i < n; i += %d)" % Z.RLC_LANES in cells and "LAUNCH(k_cells_rlc, 1, %d," % Z.RLC_LANES in cells
    capi = text("csrc", "bls_capi_kzg.hip")
    assert constant(capi, r"constexpr size_t KZG_ITEMS_MAX = (\d+);") == Z.KZG_ITEMS_MAX
    assert "launch_g1_sum_aff(st, S, live, 2 * n + 1, tmp, sums)" in capi
    assert "launch_g1_sum_aff(st, S + 2 * n + 1, live + 2 * n + 1, n, tmp, sums + 1)" in capi
    capic = text("csrc", "bls_capi_kzg_cells.hip")
    assert constant(capic, r"constexpr size_t KZC_MSM_ROWS = (\d+);") == Z.KZC_MSM_ROWS
    assert constant(capic, r"constexpr size_t KZC_ITEMS_MAX = (\d+);") == Z.KZC_ITEMS_MAX
    assert "launch_g1_sum_aff(st, S, live, nc + n + 1, tmp, sums)" in capic
    assert "launch_g1_sum_aff(st, S + nc + n + 1, live + nc + n + 1, n, tmp, sums + 1)" in capic
    # the Python limits are the C calls'
    py, pyc = text("bls_mi355x", "kzg.py"), text("bls_mi355x", "kzg_cells.py")
    assert constant(py, r"\nITEMS_MAX = (\d+)") == Z.KZG_ITEMS_MAX
    assert constant(py, r"\nMSM_ROWS_MAX = (\d+)") == constant(capi, r"constexpr size_t KZG_MSM_BMAX = (\d+);")
    assert constant(py, r"\nBLOBS_MAX = (\d+)") == constant(capi, r"constexpr size_t KZG_BLOBS_MAX = (\d+);")
    assert constant(pyc, r"\nITEMS_MAX = (\d+)") == Z.KZC_ITEMS_MAX
    assert constant(pyc, r"\nBLOBS_MAX = (\d+)") == constant(capic, r"constexpr size_t KZC_BLOBS_MAX = (\d+);")


def test_the_sizes_are_the_seams():
    """the derived lists, spelled out: a moved constant shows here as the list it changes"""
    assert Z.MSM_ROWS == (4, 5, 64, 65, 256, 257, 1024, 1025)
    assert Z.MSM_ROWS_SPECIAL == (65, 257, 1025) and Z.MSM_ROWS_DEEP == 257
    assert Z.KZG_VALID == (256, 257, 1023, 1024, 2048, 2049) and Z.KZG_FAILING == (257, 1024)
    assert Z.CELLS_VALID == (2043, 2044, 2048, 2049) and Z.CELLS_FAILING == (511, 512, 1023)
    for B in Z.MSM_ROWS:  # scan blocks of the call
        blocks = -(-Z.G1M_SLOTS * B // Z.SCAN_BLK)
        assert blocks == {4: 1, 5: 2, 64: 16, 65: 17, 256: 64, 257: 65, 1024: 256, 1025: 257}[B]
    assert [2 * n + 1 > Z.G1Q_SUM_MAX for n in Z.KZG_VALID] == [False, False, False, True, True, True]
    assert [n > Z.G1Q_SUM_MAX for n in Z.KZG_VALID] == [False, False, False, False, False, True]
    nc = Z.CELL_COMMITMENTS
    assert [nc + n + 1 > Z.G1Q_SUM_MAX for n in Z.CELLS_VALID] == [False, True, True, True]
    assert [n > Z.G1Q_SUM_MAX for n in Z.CELLS_VALID] == [False, False, False, True]
    assert [-(-n // Z.KZC_MSM_ROWS) for n in Z.CELLS_FAILING] == [1, 2, 3]
    assert max(Z.MSM_ROWS) <= Z.G1M_BMAX and max(Z.KZG_VALID) <= Z.KZG_ITEMS_MAX
    assert max(Z.CELLS_VALID) <= Z.KZC_ITEMS_MAX


# ---- the builders ----------------------------------------------------------------------------------------------------
def test_rows_with_known_sums_spot_rows_against_g1_mul():
    pts = [O.g1_decompress(p) for p in E.known_log_table()]
    assert pts[0] == O.G1_GEN
    for idx, B, zero_sum, empty in (([0, 1], 1025, {0, 64, 1024}, {3, 1023}), ([i % 3 for i in range(17)], 9, {8}, {2})):
        rows, want, nonzero = E.rows_with_known_sums(B, idx, 0x5907, zero_sum, empty)
        assert len(rows) == len(want) == B
        assert nonzero == sum(1 for row in rows for k in row for b in E.k32(k) if b)
        live = [v for v in range(B) if v not in empty]
        assert all(0 <= k < R for row in rows for k in row)
        assert min(max(rows[v]) for v in live).bit_length() > 200
        for v in sorted(zero_sum | empty) + [1, B - 2]:
            acc = None
            for e in range(3):  # sum_i k_i T[idx_i] = sum_e (sum of the k_i naming e) T[e]
                acc = O.g1_add(acc, O.g1_mul(pts[e], sum(k for i, k in zip(idx, rows[v]) if i == e) % R))
            assert O.g1_compress(acc) == want[v], v
            if v in zero_sum:
                assert want[v] == E.G1_INF and all(rows[v])
            elif v in empty:
                assert want[v] == E.G1_INF and not any(rows[v])
            else:
                assert want[v] == O.g1_compress(O.g1_mul(O.G1_GEN, v + 1))


def test_linear_items_against_known_answer_open():
    lin = K.linear_answers()
    assert len({a[2] for a in lin}) == 4
    rng = random.Random(0x0BE4)
    for a0, a1, c, proof in lin[:2]:
        ka = K.KnownAnswer([a0, a1])
        assert ka.commitment == c
        for z in (0, K.DOMAIN[16], rng.randrange(R)):
            assert ka.open(z) == ((a0 + a1 * z) % R, proof)
    items = K.batch_items(2049)
    assert len(items) == 2049 and K.batch_items(2049) is items
    assert items[36] == (K.IDENTITY48, items[36][1], 0, K.IDENTITY48) and items[15] == K.cubic_openings()[0]
    assert items[31] == K.cubic_openings()[1] and items[16 * 37 - 1][0] == K.IDENTITY48
    a0, a1, c, proof = lin[1]
    assert items[257][0] == c and items[257][3] == proof and items[257][2] == (a0 + a1 * items[257][1]) % R
    assert len({it[1] for it in items if it[0] in {a[2] for a in lin}}) > 1800  # a z of its own per linear item
    y, proof = K.known_answers()[1].open(K.CUBIC_Z[4])
    assert K.cubic_openings()[4] == (K.known_answers()[1].commitment, K.CUBIC_Z[4], y, proof)
