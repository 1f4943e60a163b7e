"""The batch sizes at which the table MSM and the KZG verification calls change shape, as the GPU tests of those
seams take them (test_gpu_g1_table_rows.py, test_gpu_kzg.py, test_gpu_cells.py).  The constants restate csrc/ and
bls_mi355x/; tests/test_seams_cpu.py reads them from the source text and fails, naming the constant, when one moves:
the sizes below then move with it.

  table MSM    a call of B rows has G1M_SLOTS B counters, scanned in blocks of SCAN_BLK; k_g1m_scan_top takes
               SCAN_TOP block totals per round and carries into the next; k_g1m_final / k_g1m_compress are blocks
               of FINAL_LANES rows
  batch sums   launch_g1_sum_aff: one workgroup up to G1Q_SUM_MAX points, two passes above
  rlc kernels  k_kzg_rlc and k_cells_rlc: one workgroup of RLC_LANES lanes striding over the items
  cells        the per-item path's interpolant commitments come in table MSMs of KZC_MSM_ROWS rows
"""
G1M_SLOTS = 256        # bucket slots per row (csrc/bls_g1_msm.h)
SCAN_BLK = 1024        # counters per scan block (csrc/bls_g1_table.hip)
SCAN_TOP = 256         # block totals per round of k_g1m_scan_top (its block size)
FINAL_LANES = 64       # rows per block of k_g1m_final and k_g1m_compress
G1M_BMAX = 65536       # rows per call (csrc/bls_capi_msm.hip)
G1Q_SUM_NT = 256       # lanes of k_g1_sum_q (csrc/bls_kernels.hip)
G1Q_SUM_MAX = 2048     # points of the one-workgroup sum: 8 per lane
RLC_LANES = 256        # KZB_LANES (csrc/bls_kzg_blob.h); k_cells_rlc strides by the same literal
KZG_ITEMS_MAX = 65536  # items per bls_kzg_verify_batch (csrc/bls_capi_kzg.hip)
KZC_MSM_ROWS = 511     # rows per table MSM of the cells' per-item path (csrc/bls_capi_kzg_cells.hip)
KZC_ITEMS_MAX = 8192   # cells per bls_kzg_verify_cells
CELL_COMMITMENTS = 4   # distinct commitments of cell_inputs.batch_items

ROWS_PER_SCAN_BLK = SCAN_BLK // G1M_SLOTS

# bls_g1_table_msm, rows per call: one and two scan blocks; one and two blocks of the final kernels; one and two
# 256-row groups; a full round of k_g1m_scan_top and a second round with a carry
MSM_ROWS = (ROWS_PER_SCAN_BLK, ROWS_PER_SCAN_BLK + 1, FINAL_LANES, FINAL_LANES + 1, 256, 257,
            SCAN_TOP * ROWS_PER_SCAN_BLK, SCAN_TOP * ROWS_PER_SCAN_BLK + 1)
MSM_ROWS_SPECIAL = (FINAL_LANES + 1, 257, SCAN_TOP * ROWS_PER_SCAN_BLK + 1)  # the cases with identity and empty rows
MSM_ROWS_DEEP = 257  # the rows of the case with a second fold level

# bls_kzg_verify_batch, items per call: the rlc stride; the first sum (2 n + 1 points) and the second (n points)
# on both sides of G1Q_SUM_MAX
KZG_VALID = (RLC_LANES, RLC_LANES + 1, (G1Q_SUM_MAX - 1) // 2, (G1Q_SUM_MAX - 1) // 2 + 1, G1Q_SUM_MAX,
             G1Q_SUM_MAX + 1)
KZG_FAILING = (RLC_LANES + 1, (G1Q_SUM_MAX - 1) // 2 + 1)
KZG_BAD_AT = (0, RLC_LANES - 1, RLC_LANES, -1)

# bls_kzg_verify_cells with CELL_COMMITMENTS distinct commitments: the first sum has nc + n + 1 points, the second n
CELLS_VALID = (G1Q_SUM_MAX - CELL_COMMITMENTS - 1, G1Q_SUM_MAX - CELL_COMMITMENTS, G1Q_SUM_MAX, G1Q_SUM_MAX + 1)
CELLS_FAILING = (KZC_MSM_ROWS, KZC_MSM_ROWS + 1, 2 * KZC_MSM_ROWS + 1)  # one chunk, a second, a third
CELLS_BAD_AT = (0, KZC_MSM_ROWS - 1, KZC_MSM_ROWS, -1)
