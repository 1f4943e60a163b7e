// C ABI, the FAV (FastAggregateVerify) batch pipeline: the forms of a batch (FavItems), the stream plan
// (fav_prepare) and its stages, the bisection fallback, the host-buffer entry points and the pipelined job API.
#include "bls_capi_internal.h"

// The items of one FAV batch, in whichever form.  fav_prepare and job_submit take device pointers; fav_batch_host
// takes the same descriptor over host buffers and hands fav_prepare its device copies.
//   signers: index lists (idx / offs), or -- bits non-null -- (committees, participation bits) over the context's
//     committee table.  bits_plan has then checked the arguments and left the host tables in the job; a pre-stage
//     expands every item into the list its gather adds, and the gather variant of bls_gather_bits.hip writes the
//     same apka / gstat the index gather would have written for the expanded list.  Nothing after them knows the
//     difference.  Or -- keys non-null, never together with bits -- index lists into a table of K compressed keys
//     that belongs to the batch: a pre-stage decodes and KeyValidates it into the job's own RegKey records
//     (S_KTAB), and the index gather runs on those records and K in place of the registry and its size.  No
//     registry is needed or touched.
//   messages: one per item, or -- msg_id non-null (host, B entries) -- a table of M messages of which item i signs
//     entry msg_id[i].  The per-item stages (gather, decode, r_i apk_i chains, MSM) run over the B items as ever;
//     the per-message stages (hash_to_G2, G2 lines, f accumulation) run over M + MSM_UPAIRS pairs whose G1 side is
//     the segmented sum of the items' r_i apk_i (bls_g1_segsum.h), and the kernel-form thresholds key on M.
struct BitsArgs {
  const uint8_t* bits;  // the items' bit bytes, item b at bit_offs[b]
  size_t bytes;         // their total (fav_batch_host's upload)
  int mode;
};
struct KeyTable {
  const uint8_t* keys48;  // K compressed keys
  size_t K;
  uint8_t* valid;  // nullable: the KeyValidate verdict per entry, one byte each
};
struct FavItems {
  size_t B;
  const uint32_t* idx;
  const uint64_t* offs;
  const BitsArgs* bits;
  const uint8_t* msgs;  // 32 bytes each
  size_t M;
  const uint32_t* msg_id;
  const uint8_t* sigs;  // 96 bytes each
  const uint8_t* seed32;  // host: the RLC seed
  const KeyTable* keys = nullptr;
  bool shared() const { return msg_id != nullptr; }
  size_t NH() const { return shared() ? M : B; }  // messages hashed = pairs of the H side
  // pairs 0 .. NH: (r_i apk_i, H_i); pairs NH .. NH + 64: (-w_b G1, U_b), the MSM's bit-sums (bls_msm.hip).  The 64
  // scalar bits read as r_i = a + b lambda (a the low, b the high half; lambda = -x^2 mod r, phi's eigenvalue on
  // G1): bit b weighs w_b = 2^b below 32 and 2^(b - 32) lambda above, on both sides (bls_g1_endo.h, the comb)
  size_t NP() const { return NH() + MSM_UPAIRS; }
};

// The scratch of one batch (fav_scratch fills it, the stages read it).
struct FavScratch {
  int *status, *gstat, *flag, *dstat, *redo;
  G1P *apka, *rpj, *gsum, *sega, *segb;
  G1A* rP;
  G2A *sig, *H;
  Fp12 *f, *ft, *fo;
  Fd *msmf, *hcf;
  uint64_t *rsc, *tab;
  uint32_t *msmu, *mlines, *seg_items, *msgid, *list, *gaff;
  uint8_t* seed;
  SegRun* runs;
  BitsItem* bitems;
  RegKey* ktab;
  // the Miller pairs' status and G1 side: the item arrays themselves, [0, B) items then the MSM pairs -- or, shared,
  // arrays of their own, [0, M) group sums then the MSM pairs, beside item arrays of B
  int* pstat;
  G1A* pP;
};

int capi::host_seed(bls_ctx* ctx, uint8_t seed[32]) {
  if (bls_host_seed(seed) != 0) {
    ctx->err = "could not read 32 bytes of entropy for the RLC seed";
    return BLS_E_DEVICE;
  }
  return 0;
}

extern "C" {

// The host half of a bits batch, before any device call: every committee id names a table entry, item b carries
// exactly ceil(n_b / 8) bytes (n_b the members of its committees), and the table is the registry's.  Leaves the
// job-owned copies (committee ids rebased to 0, comm_offs | bit_offs | slot_offs) that fav_prepare uploads.
static int bits_plan(bls_ctx* ctx, const uint32_t* comm_ids, const uint64_t* comm_offs, const uint64_t* bit_offs,
                     size_t B, int mode) {
  if (!ctx->ctab_loaded) {
    ctx->err = "no committee table loaded (bls_committees_load)";
    return BLS_E_ARG;
  }
  if (ctx->ctab_gen != ctx->reg_gen) {
    ctx->err = "the committee table is stale: the registry was replaced after bls_committees_load";
    return BLS_E_ARG;
  }
  if (mode != BITS_MODE_AUTO && mode != BITS_MODE_DIRECT && mode != BITS_MODE_COMPLEMENT) {
    ctx->err = "mode must be 0 (auto), 1 (direct) or 2 (complement)";
    return BLS_E_ARG;
  }
  if (!comm_offs || !bit_offs) return BLS_E_ARG;
  const size_t C = ctx->ctab_offs_h.size() - 1;
  const uint64_t c0 = comm_offs[0];
  for (size_t b = 0; b < B; b++)
    if (comm_offs[b + 1] < comm_offs[b] || bit_offs[b + 1] < bit_offs[b]) return BLS_E_ARG;
  const uint64_t ncomm = comm_offs[B] - c0;
  if (ncomm && !comm_ids) return BLS_E_ARG;
  Job& J = *ctx->j;
  std::vector<uint64_t>& n = J.bits_n;
  n.resize(B);
  for (size_t b = 0; b < B; b++) {
    n[b] = 0;
    for (uint64_t j = comm_offs[b]; j < comm_offs[b + 1]; j++) {
      const uint32_t c = comm_ids[j];
      if (c >= C) {
        ctx->err = "committee id out of range";
        return BLS_E_ARG;
      }
      n[b] += ctx->ctab_offs_h[c + 1] - ctx->ctab_offs_h[c];
    }
    if (n[b] > 0xffffffffull || bit_offs[b + 1] - bit_offs[b] != (n[b] + 7) / 8) {
      ctx->err = "an item needs ceil(n / 8) bytes of bits for the n members of its committees";
      return BLS_E_ARG;
    }
  }
  // the arguments stand: now the job's tables (an upload still in flight reads the old ones)
  J.bits_B = 0;
  if (J.bits_up_pending) {
    HIPCK(hipEventSynchronize(J.ev[EV_BITS]));
    J.bits_up_pending = false;
  }
  const size_t bytes = 3 * (B + 1) * 8 + ncomm * 4;
  if (J.bits_tab_cap < bytes) {
    if (J.bits_tab) HIPCK(hipHostFree(J.bits_tab));
    J.bits_tab = nullptr;
    J.bits_tab_cap = 0;
    HIPCK(hipHostMalloc((void**)&J.bits_tab, bytes + bytes / 4, hipHostMallocDefault));
    J.bits_tab_cap = bytes + bytes / 4;
  }
  J.bits_tab_bytes = bytes;
  uint64_t* co = J.bits_tab;
  uint64_t *bo = co + (B + 1), *so = bo + (B + 1);
  so[0] = 0;
  for (size_t b = 0; b < B; b++) so[b + 1] = so[b] + n[b];
  for (size_t b = 0; b <= B; b++) {
    co[b] = comm_offs[b] - c0;
    bo[b] = bit_offs[b];
  }
  if (ncomm) memcpy(so + (B + 1), comm_ids + c0, ncomm * 4);
  return 0;
}

// Every scratch slot of the batch, sized by its form, before anything is enqueued.
static int fav_scratch(bls_ctx* ctx, const FavItems& it, FavScratch& S) {
  const size_t B = it.B, NH = it.NH(), NP = it.NP();
  S = FavScratch{};
  SCR(S_STATUS, it.shared() ? B : NP, S.status);
  SCR(S_GSTAT, B, S.gstat);
  SCR(S_APKA, B, S.apka);
  SCR(S_SIG, B, S.sig);
  SCR(S_RP, it.shared() ? B : NP, S.rP);
  SCR(S_H, NP, S.H);
  SCR(S_FLAG, NH, S.flag);
  SCR(S_RSC, B, S.rsc);
  SCR(S_MSMU, msm_scratch_u32(B), S.msmu);
  SCR(S_MSMF, msm_scratch_fd(B), S.msmf);
  SCR(S_HCF, h2c_scratch_fd(NH), S.hcf);
  SCR(S_RPJ, B, S.rpj);
  S.pstat = S.status;
  S.pP = S.rP;
  if (it.shared()) {
    const SegPlan& sp = ctx->j->seg;
    SCR(S_PSTAT, NP, S.pstat);
    SCR(S_GP, NP, S.pP);
    SCR(S_GSUM, it.M, S.gsum);
    SCR(S_SEGA, sp.max_tmp(), S.sega);
    SCR(S_SEGB, sp.levels() > 1 ? sp.level_tmp[1] : 0, S.segb);
    SCR(S_SEGRUN, sp.runs.size(), S.runs);
    SCR(S_SEGIT, B, S.seg_items);
    SCR(S_MSGID, B, S.msgid);
  }
  if (!knobs().miller_fused) SCR(S_MLINES, miller_lines_u32(NP), S.mlines);
  SCR(S_MSTAT, B, S.dstat);
  SCR(S_FAV_F, NP, S.f);  // per-item (or per-group) f, kept for the bisection: not S_F, which per-call checks use
  SCR(S_FAV_FT, NP / 8 + 16, S.ft);
  SCR(S_FPART, 1, S.fo);
  SCR(S_SEED, 32, S.seed);
  if (it.bits) {
    const Job& J = *ctx->j;
    SCR(S_BTAB, (J.bits_tab_bytes + 7) / 8, S.tab);
    SCR(S_BLIST, J.bits_tab[3 * (B + 1) - 1], S.list);
    SCR(S_BITEM, B, S.bitems);
  } else if (it.keys) {
    SCR(S_KTAB, it.keys->K ? it.keys->K : 1, S.ktab);  // record 0 exists for any K (keys_stage)
  } else if (const char* gv = getenv("BLS_GATHER"); gv && !strcmp(gv, "affine") && fav_gather_aff_words(B)) {
    SCR(S_GAFF, fav_gather_aff_words(B), S.gaff);  // read per batch (gather_stage)
    SCR(S_GREDO, B, S.redo);
  }
  return 0;
}

// A shared batch's host plan, before any device call: a bad id is refused here.
static int shared_plan(bls_ctx* ctx, const FavItems& it) {
  Job& J = *ctx->j;
  if (!seg_plan(it.msg_id, it.B, it.M, J.seg)) {
    ctx->err = "msg_id out of range (or an empty message table)";
    return BLS_E_ARG;
  }
  J.seg_ids.assign(it.msg_id, it.msg_id + it.B);
  return 0;
}

// the grouping's tables on stream1, behind anything (a bisection's per-item H gather) that still reads the
// previous ids; the branches then fork from here, not from a bisection's EV_BIS
static int shared_uploads(bls_ctx* ctx, const FavItems& it, const FavScratch& S, hipStream_t st) {
  Job& J = *ctx->j;
  const SegPlan& sp = J.seg;
  HIPCK(hipMemcpyAsync(S.msgid, J.seg_ids.data(), it.B * 4, hipMemcpyHostToDevice, st));
  HIPCK(hipMemcpyAsync(S.seg_items, sp.grp_items.data(), it.B * 4, hipMemcpyHostToDevice, st));
  HIPCK(hipMemcpyAsync(S.runs, sp.runs.data(), sp.runs.size() * sizeof(SegRun), hipMemcpyHostToDevice, st));
  J.bis_pending = false;
  return 0;
}

// the branches fork from stream1's tail -- or, after a bisection still running there, from the point where it
// has copied everything it reads of the state stream2 / stream3 write (fav_bisect)
static int fork_stage(bls_ctx* ctx, hipStream_t st, hipStream_t st2, hipStream_t st3) {
  Job& J = *ctx->j;
  hipEvent_t fork = J.ev[EV_FORK];
  if (J.bis_pending) {
    fork = J.ev[EV_BIS];
    J.bis_pending = false;
  } else {
    HIPCK(hipEventRecord(fork, st));
  }
  HIPCK(hipStreamWaitEvent(st2, fork, 0));
  if (st3 != st2) HIPCK(hipStreamWaitEvent(st3, fork, 0));
  return 0;
}

// (committees, bits) items, the pre-stage: the job's tables up in one copy, then one wave per item expands it
// into its index list at the slot the host computed (the prefix sum of the member counts).  On stream2, in
// front of the hash -- whose chain waits for the MSM anyway -- so that the expansion runs beside the signature
// decode instead of in front of the gather: a job's latency, which a fixed pipeline depth turns into
// throughput, stays what the index form's is.  The gather waits for EV_BITS.
static int bits_stage(bls_ctx* ctx, const FavItems& it, const FavScratch& S, hipStream_t st2) {
  Job& J = *ctx->j;
  const size_t B = it.B;
  HIPCK(hipMemcpyAsync(S.tab, J.bits_tab, J.bits_tab_bytes, hipMemcpyHostToDevice, st2));
  const uint32_t* d_comm = reinterpret_cast<const uint32_t*>(S.tab + 3 * (B + 1));
  PROF2(P_BITS_EXPAND, st2, launch_bits_expand(st2, B, it.bits->mode, d_comm, S.tab, it.bits->bits, S.tab + (B + 1),
                                               S.tab + 2 * (B + 1), ctx->ctab_idx, ctx->ctab_offs, ctx->ctab_stat,
                                               S.list, S.bitems));
  return 0;
}

// A batch's own key table, the pre-stage of the keys form: the K compressed keys decoded and KeyValidated into the
// job's RegKey records, verdict in REG_VALID as the registry stores it, by the KeyValidate kernels' record output
// (launch_key_table: one launch, no G1A / ok arrays and no pack launch in between).  On stream1 in front of the gather,
// its only reader: the hash on stream2 has forked already and does not wait for it, and the table is the job's
// (S_KTAB), so ten jobs in flight keep ten tables.  The gather loads record 0 for an index out of range, whatever K
// is: with K == 0 that record is zeroed, a key that is not valid.
static int keys_stage(bls_ctx* ctx, const FavItems& it, const FavScratch& S, hipStream_t st) {
  const KeyTable& kt = *it.keys;
  if (!kt.K) {
    HIPCK(hipMemsetAsync(S.ktab, 0, sizeof(RegKey), st));
    return 0;
  }
  PROF2(P_KEY_VALIDATE, st, launch_key_table(st, kt.keys48, kt.K, S.ktab, kt.valid));
  return 0;
}

static int hash_stage(bls_ctx* ctx, const FavItems& it, const FavScratch& S, hipStream_t st2) {
  PROF2(P_FAV_HASH, st2, launch_h2c(st2, it.NH(), it.msgs, nullptr, S.hcf, S.H, S.flag));
  return h2c_fallback(ctx, st2, it.NH(), it.msgs, nullptr, S.flag, S.H);
}

static int decode_stage(bls_ctx* ctx, const FavItems& it, const FavScratch& S, hipStream_t sd) {
  if (it.shared())
    PROF2(P_SIG_DECODE, sd, launch_sig_decode_idx(sd, it.B, it.msgs, S.msgid, it.sigs, S.seed, S.sig, S.rsc, S.dstat));
  else
    PROF2(P_SIG_DECODE, sd, launch_sig_decode(sd, it.B, it.msgs, it.sigs, S.seed, S.sig, S.rsc, S.dstat));
  return 0;
}

// the registry gather: the complete-formula kernel (k_fav_gather_q: two keys of a lane summed first, then one
// complete addition; 4 lanes per aggregate from 4,096 aggregates up, 16 from 1,024, else 64; 230 registers by the
// compiler's report, two waves per SIMD), or with BLS_GATHER=affine (read per batch) affine additions sharing one
// inversion per level (bls_gather_aff.hip: 42 % fewer VALU instructions per aggregate than the 16-lane kernel had
// then, 234 registers; C2 measured the same within +-1 % over three A/Bs, profiles/r06_gather_ab.txt); aggregates
// with an exceptional pair are redone by the complete formulas.  The gather is not free: it was 2,500 waves of a
// C2 batch, 30 % of the instructions the batch issued and about a quarter of a C2 step (C2 / C4 =
// 1.39 per item, the work model's 1.38).  The affine
// A/B did not show that because its waves held their SIMDs alone, 28.5 % of the time waiting on HBM level lists
// (~790 exclusive SIMD-ms, as much as it saved); cutting the complete kernel's own instructions by 15.8 % (one
// reduction per output coordinate, bls_fq_g1.h) gained C2 3.1 % (profiles/g1dot_ab.txt), and by a further 20 %
// (625 waves of 584,671 for 2,500 of 183,088: pair sums, four lanes) 3.3 % (profiles/gather_pairs_ab.txt).
static int gather_stage(bls_ctx* ctx, const FavItems& it, const FavScratch& S, hipStream_t st) {
  Job& J = *ctx->j;
  const size_t B = it.B;
  // the keys form gathers from the job's table (keys_stage) with the complete formulas, as the bits form does
  const RegKey* reg = it.keys ? S.ktab : ctx->reg;
  const uint32_t nreg = (uint32_t)(it.keys ? it.keys->K : ctx->reg_n);
  if (it.bits) {
    // the gather variant sums the expanded lists -- and, for complement items, subtracts them from the committees'
    // cached sums.  The affine gather has no such form.
    PROF(P_FAV_GATHER, launch_fav_gather_bits(st, S.list, S.bitems, B, ctx->reg, nreg,
                                              reinterpret_cast<const uint32_t*>(S.tab + 3 * (B + 1)), S.tab,
                                              ctx->ctab_sum, S.apka, S.gstat, nullptr));
    J.bits_B = B;
    J.bits_items = S.bitems;
    ctx->work_job = &J;
  } else if (S.gaff) {
    PROF(P_FAV_GATHER, launch_fav_gather_aff(st, it.idx, it.offs, B, reg, nreg, S.apka, S.gstat, S.gaff, S.redo));
    HIPCK(launch_fav_gather_redo(st, it.idx, it.offs, B, reg, nreg, S.apka, S.gstat, S.redo));
  } else {
    PROF(P_FAV_GATHER, launch_fav_gather(st, it.idx, it.offs, B, reg, nreg, S.apka, S.gstat));
  }
  return 0;
}

// The MSM covers every decoded signature of a valid aggregate key, before
// the subgroup checks: a decodable signature outside G2 stays in S, so the
// batch check fails and fav_finish re-checks every item individually.  It
// reads only gstat (gather) and dstat (decode), which no kernel writes
// after EV_GATHER / EV_SIG; the subgroup verdicts go to `status`, written on
// stream1 while (or after) the MSM runs.
static int msm_stage(bls_ctx* ctx, const FavItems& it, const FavScratch& S, hipStream_t sm) {
  const size_t NH = it.NH();
  PROF2(P_MSM, sm, launch_msm_upairs(sm, it.B, S.gstat, S.dstat, S.rsc, S.sig, S.msmu, S.msmf, ctx->comb, S.pP + NH,
                                     S.H + NH, S.pstat + NH));
  return 0;
}

// A FAV batch's Miller loops run split -- the line kernel (k_miller_lines2) over all NP pairs on stream2 right after
// the hash and the MSM, the f accumulation on stream1 -- or, with BLS_MILLER_FUSED=1, as one fused kernel
// (k_miller_fused, lines in LDS) on stream1.  The fused kernel holds a SIMD per
// line wave for the whole loop, so per batch it costs more SIMD time than the two kernels at full occupancy (C2
// 2.32 -> 2.14 M FAV/s, C3 1.51 -> 1.46 M: profiles/r05o_miller_fused_ab.txt) although its launch alone runs the
// Miller loop at 0.0995 of peak against the accumulation kernel's 0.070; the latency-bound callers -- the
// bisection's per-item values and AggregateVerify batches -- always take it.
static int lines_stage(bls_ctx* ctx, const FavItems& it, const FavScratch& S, hipStream_t st2) {
  PROF2(P_MILLER_LINES, st2, launch_miller_lines(st2, S.H, it.NP(), S.mlines));
  return 0;
}

// the subgroup checks and the r_i apk_i chains; shared, then the segmented sum of the items' affine r_i apk_i into
// one point per message: a launch per fold level, the partial arrays alternating, then the M sums to affine (ok 0 --
// an empty, rejected or cancelling group -- gives .inf, a dead pair whose factor is 1)
static int chains_stage(bls_ctx* ctx, const FavItems& it, const FavScratch& S, hipStream_t st) {
  PROF(P_SIG_VM, launch_sig_vm(st, it.B, S.gstat, S.status, S.dstat, S.apka, S.sig, S.rsc, S.rpj, S.rP));
  if (!it.shared()) return 0;
  const SegPlan& sp = ctx->j->seg;
  for (size_t l = 0; l < sp.levels(); ++l) {
    const uint32_t n = sp.level_off[l + 1] - sp.level_off[l];
    G1P *in = (l & 1) ? S.sega : S.segb, *out = (l & 1) ? S.segb : S.sega;
    HIPCK(launch_g1_seg_fold(st, (int)l, S.runs + sp.level_off[l], n, S.seg_items, S.status, S.rP, in, out, S.gsum,
                             S.pstat));
  }
  HIPCK(launch_g1_affine(st, it.M, S.pstat, S.gsum, S.pP));
  return 0;
}

// f accumulated over all NP pairs by k_miller_acc4q (four lanes per f, G pairs per f: one squaring per step for all
// G); *mg = the pairs per f.
// four pairs share each f (one squaring per step for all four) on full batches: the least work per pair, and
// the pipeline is bound by work (C2 +3.0 % over two pairs per f, profiles/r06a_g4_ab.txt, although the launch
// fills only 0.15 of the SIMDs); below ACC_SHARED_MIN (4,096) items the launch under-fills the chip and the chain
// latency is what counts, so one pair per f (a step is a squaring and ONE line: ~37 % shorter chains for ~24 % more
// products).  Knob BLS_ACC_G = 1 / 2 / 4 / 8.
// knob BLS_ACC_LL = 1: G = 4 with each step's four lines multiplied together before they meet f
// (k_miller_acc4l: 12 Fp2 products per lane per round of four lines instead of 16, but the Karatsuba sums'
// normalisations, selects and exchanges leave it 3 % fewer VALU instructions, 13 % waiting, 5.10 ms per launch
// against 4.81: profiles/r06u_acc_ll_ab.txt)
// below ACC8_MAX (2,048) items one pair per f runs on eight lanes (k_miller_acc8: ~40 % fewer product rounds per step
// for twice the waves): a latency win for the small batches whose chain decides (C5's 1,024: +2.4 %), a loss where
// the SIMD time does (C3's 2,048: -8.6 %; profiles/r06y_acc8_ab.txt).  Knob BLS_ACC8_MAX.
static int acc_stage(bls_ctx* ctx, const FavItems& it, const FavScratch& S, hipStream_t st, int* mg_out) {
  const Knobs& k = knobs();
  const size_t NH = it.NH(), NP = it.NP();
  const int mg = NH >= k.acc_shared_min ? (k.acc_g == 8 || k.acc_g == 4 || k.acc_g == 1 ? k.acc_g : 2) : 1;
  *mg_out = mg;
  if (k.miller_fused)
    PROF(P_MILLER, launch_miller_fused(st, S.pP, S.H, S.pstat, NP, S.f, mg));
  else if (mg == 1 && NH < k.acc8_max)
    PROF(P_MILLER, launch_miller_acc8(st, S.pP, S.H, S.pstat, NP, S.mlines, miller_lines_ld(NP), S.f));
  else if (mg == 4 && k.acc_ll)
    PROF(P_MILLER, launch_miller_acc4l(st, S.pP, S.H, S.pstat, NP, S.mlines, miller_lines_ld(NP), S.f));
  else
    PROF(P_MILLER, launch_miller_acc4(st, S.pP, S.H, S.pstat, NP, S.mlines, miller_lines_ld(NP), S.f, mg));
  return 0;
}

// Branches, three streams:
//   stream1: registry gather (affine apk) -> subgroup / r_i apk_i chains -> f accumulation
//   stream2: hash_to_G2 of every message -> (after the MSM) the G2 lines of all NP pairs
//   stream3: signature decompression + RLC scalars -> MSM bit-sums U_b of S = sum r_i sigma_i
// two streams (stream3 == stream2, BLS_JOB_STREAMS=2, the default): stream3's work on stream1 (decode before the
// gather, MSM after it), off the hash -> lines chain of stream2
// a keys batch: its key-table stage on stream1 in front of the gather (keys_stage), after the hash has been enqueued
static int fav_prepare(bls_ctx* ctx, const FavItems& it, Fp12** out_f) {
  if (!it.keys && (!ctx->reg || !ctx->reg_n)) {  // index lists and bits read the registry; a keys batch brings its table
    ctx->err = "no registry loaded";
    return BLS_E_NOREG;
  }
  if (it.keys && (it.bits || it.keys->K > 0xffffffffull || (it.keys->K && !it.keys->keys48))) return BLS_E_ARG;
  Job& J = *ctx->j;
  if (it.shared()) CK(shared_plan(ctx, it));
  FavScratch S;
  CK(fav_scratch(ctx, it, S));
  hipStream_t st = J.stream, st2 = J.stream2, st3 = J.stream3;
  CK(ensure_comb(ctx, st));
  // the job's own-product verdict belongs to the batch job_submit prepares; any other batch prepared on this slot
  // (the host-buffer calls on job 0) invalidates it
  J.own_pending = false;
  J.own_state = -1;
  J.comm_pending = false;
  const bool two = st3 == st2, fused = knobs().miller_fused;
  hipStream_t sd = two ? st : st3;  // the decode's and the MSM's stream
  if (it.shared()) CK(shared_uploads(ctx, it, S, st));
  J.fav_shared = it.shared();
  // the seed goes on the decode's stream, its reader, so the fork need not follow stream1
  HIPCK(hipMemcpyAsync(S.seed, it.seed32, 32, hipMemcpyHostToDevice, sd));
  CK(fork_stage(ctx, st, st2, st3));
  if (it.bits) {
    CK(bits_stage(ctx, it, S, st2));
    HIPCK(hipEventRecord(J.ev[EV_BITS], st2));
    J.bits_up_pending = true;
  }
  CK(hash_stage(ctx, it, S, st2));
  if (it.keys) CK(keys_stage(ctx, it, S, st));
  CK(decode_stage(ctx, it, S, sd));
  HIPCK(hipEventRecord(J.ev[EV_SIG], sd));
  if (it.bits) HIPCK(hipStreamWaitEvent(st, J.ev[EV_BITS], 0));
  CK(gather_stage(ctx, it, S, st));
  HIPCK(hipEventRecord(J.ev[EV_GATHER], st));
  if (!two) HIPCK(hipStreamWaitEvent(sd, J.ev[EV_GATHER], 0));
  CK(msm_stage(ctx, it, S, sd));
  HIPCK(hipEventRecord(J.ev[EV_MSM], sd));
  if (!fused) {
    HIPCK(hipStreamWaitEvent(st2, J.ev[EV_MSM], 0));
    CK(lines_stage(ctx, it, S, st2));
  }
  HIPCK(hipEventRecord(J.ev[EV_JOIN], st2));
  if (!two) HIPCK(hipStreamWaitEvent(st, J.ev[EV_SIG], 0));
  CK(chains_stage(ctx, it, S, st));
  HIPCK(hipStreamWaitEvent(st, J.ev[EV_JOIN], 0));
  if (fused && !two) HIPCK(hipStreamWaitEvent(st, J.ev[EV_MSM], 0));
  CK(acc_stage(ctx, it, S, st, &J.fav_mg));
  PROF(P_FP12_PROD, launch_fp12_prod_vm(st, S.f, (it.NP() + J.fav_mg - 1) / J.fav_mg, S.ft, S.fo));  // the product
  ctx->last_hashes = it.NH();
  ctx->last_pairs = it.NP();
  J.fav_B = it.B;
  J.fav_ready = true;
  *out_f = S.fo;
  return 0;
}


// Bisection fallback ("a failing batch falls back to
// per-signature bisection"), on the job's own stream with no host round trip.
// The leaves are the items' Miller values from the batch's own kernels:
//   f_H,i   = ML(r_i apk_i, H_i): the batch's per-item f (one pair per f below
//             ACC_SHARED_MIN items) or k_miller_fused<1> over the batch's
//             r_i apk_i and H_i again (shared-f batches);
//   f_sig,i = ML(-r_i G1, sigma_i): -r_i G1 from a fixed-base comb (8 mixed
//             additions, k_neg_rg1; its upper four windows hold phi images, so
//             r_i = a + b lambda as in the batch), f by k_miller_fused<1>;
// leaf_i = f_H,i f_sig,i, and a 16-ary product tree above the leaves.  A node's
// check is FE(node) == 1: the product of e(r_i apk_i, H_i) e(-r_i G1, sigma_i)
// over its items, the random linear combination of their checks.  The first
// checked level is the lowest with at most 64 nodes (all of them checked; the
// root first when the caller does not know it fails); every level below is one
// launch of k_fe_check_gated that checks exactly the nodes whose parent failed,
// reading the parent's result on the device.  A leaf that fails is an invalid
// item; every item under a passing node keeps its per-item status.  With k bad
// items among B this is ~64 + 16 k (log16(B) - 2) checks.  Items with status 0
// (rejected before the pairing) have leaf 1 and keep verdict 0.  root_bad: the
// caller already knows the product fails.
static int fav_bisect(bls_ctx* ctx, bool root_bad, uint8_t* d_out) {
  Job& J = *ctx->j;
  const size_t B = J.fav_B;
  const int* status = (const int*)J.buf[S_STATUS].p;
  const uint64_t* rsc0 = (const uint64_t*)J.buf[S_RSC].p;
  const G1A* rP = (const G1A*)J.buf[S_RP].p;
  const G2A* H = (const G2A*)J.buf[S_H].p;  // per item; per message for a shared-message batch (H_item below)
  const G2A* sig0 = (const G2A*)J.buf[S_SIG].p;
  Fp12* fb = (Fp12*)J.buf[S_FAV_F].p;
  std::vector<size_t> off{0}, cnt{B};
  while (cnt.back() > 1) {
    off.push_back(off.back() + cnt.back());
    cnt.push_back((cnt.back() + 15) / 16);
  }
  const int R = (int)cnt.size() - 1;
  int T = 0;  // first checked level below the root: the lowest with at most 64 nodes
  while (T < R && cnt[T] > 64) T++;
  const int top = root_bad ? T : R;  // highest level the tree must be built to
  const size_t total = off[top] + cnt[top];
  G1A* Ps;
  G1P* Pj;
  Fp12 *fS, *fH, *tree;
  int* res;
  uint32_t* nchk;
  G2A* sig;
  uint64_t* rsc;
  SCR(S_BP, B, Ps);
  SCR(S_BQ, B, Pj);
  SCR(S_BS, B, fS);
  SCR(S_BT, total, tree);
  SCR(S_BRES, total, res);
  SCR(S_BBAD, 1, nchk);
  SCR(S_BSIG, B, sig);
  SCR(S_BRSC, B, rsc);

  // per-item f_H: the batch's own f (one pair per f), else recomputed -- always for a shared-message batch, whose
  // pairs are per message: over the items' r_i apk_i and H_item[i] = H[msg_id[i]]
  const bool refH = J.fav_mg > 1 || J.fav_shared;
  G2A* Hit = nullptr;
  if (J.fav_shared) SCR(S_BHIT, B, Hit);
  if (refH) SCR(S_BSEL, B, fH);
  else fH = fb;
  hipStream_t st = J.stream;
  // first everything read of the state that the job's next batch writes from stream2 / stream3 (H and the line
  // records, sigma_i, r_i); that batch forks from ev_bis (fav_prepare) while the rest runs here
  if (J.fav_shared) {
    HIPCK(launch_g2a_gather(st, B, H, (const uint32_t*)J.buf[S_MSGID].p, Hit));
    H = Hit;
  }
  if (refH) HIPCK(launch_miller_fused(st, rP, H, status, B, fH, 1));
  HIPCK(hipMemcpyAsync(sig, sig0, B * sizeof(G2A), hipMemcpyDeviceToDevice, st));
  HIPCK(hipMemcpyAsync(rsc, rsc0, B * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
  HIPCK(hipEventRecord(J.ev[EV_BIS], st));
  J.bis_pending = true;
  HIPCK(launch_neg_rg1(st, B, status, rsc, ctx->comb, Pj, Ps));
  HIPCK(launch_miller_fused(st, Ps, sig, status, B, fS, 1));
  HIPCK(launch_fp12_chunk_prod2(st, fH, fS, B, 1, tree));
  for (int L = 0; L < top; L++) HIPCK(launch_fp12_chunk_prod(st, tree + off[L], cnt[L], 16, tree + off[L + 1]));
  HIPCK(hipMemsetAsync(nchk, 0, sizeof(uint32_t), st));
  // the gated levels on the one-wave k_fe_check (chip time: with ten jobs in flight, C5 578k vs 519k FAV/s on the
  // six-wave k_fe_wide, profiles/r05k_c5_bisect_fe_ab.txt) or, BLS_BISECT_FE=wide, on k_fe_wide (latency)
  auto gated = knobs().bisect_fe_wide ? launch_fe_wide_gated : launch_final_check_gated;
  uint64_t rounds = 0;
  const int* parent = nullptr;
  uint32_t pdiv = 1;
  if (!root_bad && T < R) {  // the root first; level T then runs only if it failed
    HIPCK(gated(st, tree + off[R], 1, nullptr, 1, res + off[R], nchk));
    parent = res + off[R];
    pdiv = (uint32_t)cnt[T];
    rounds++;
  }
  for (int L = T; L >= 0; L--) {
    HIPCK(gated(st, tree + off[L], cnt[L], parent, pdiv, res + off[L], nchk));
    parent = res + off[L];
    pdiv = 16;
    rounds++;
  }
  HIPCK(launch_verdicts_res(st, status, res, B, d_out));
  J.bis_rounds = rounds;
  J.bis_dev_checks = nchk;  // read (after the stream) by bls_last_fallback_stats
  ctx->stats_job = &J;
  return 0;
}

static int fav_finish(bls_ctx* ctx, int batch_ok, bool root_bad, uint8_t* d_out) {
  if (!ctx->j->fav_ready) {
    ctx->err = "no prepared FAV batch";
    return BLS_E_ARG;
  }
  size_t B = ctx->j->fav_B;
  if (!B) return 0;  // an empty shard (job_submit with the device exchange): no verdicts
  int* status = (int*)ctx->j->buf[S_STATUS].p;
  if (batch_ok) {
    ctx->j->bis_checks = ctx->j->bis_rounds = 0;
    ctx->j->bis_dev_checks = nullptr;
    ctx->stats_job = ctx->j;
    PROF(P_FAV_FINISH, launch_status_to_u8(ctx->j->stream, status, B, d_out));
    return 0;
  }
  return fav_bisect(ctx, root_bad, d_out);
}

// Entropy source of the RLC seeds; only bls_set_entropy_source (a test hook) changes it.
static char g_entropy_path[256] = "/dev/urandom";

int bls_set_entropy_source(const char* path) {
  if (!path || strlen(path) >= sizeof(g_entropy_path)) return BLS_E_ARG;
  strcpy(g_entropy_path, path);
  return 0;
}

// RLC scalars must be unpredictable to whoever produced the signatures (hard part 6): a short
// read fails the call closed (BLS_E_DEVICE) instead of continuing with a predictable seed.
int bls_host_seed(uint8_t* seed32) {
  if (!seed32) return BLS_E_ARG;
  FILE* f = fopen(g_entropy_path, "rb");
  size_t got = f ? fread(seed32, 1, 32, f) : 0;
  if (f) fclose(f);
  if (got != 32) {
    memset(seed32, 0, 32);
    return BLS_E_DEVICE;
  }
  return 0;
}

// One host-buffer FAV batch: copies in, RLC batch check, bisection on failure.  h: the batch over the caller's host
// buffers (seed32 unused); for a bits batch bits_plan has run, and the bit bytes go up in the index list's place;
// a keys batch's key bytes go up into a slot of their own (S_IN0 still carries its index list) and its verdict bytes,
// when asked for, come back with the verdicts.  d_msgs / d_keys (nullable): the messages / key bytes are on the
// device already, on stream1 (bls_deposits_verify computes the one from the other there)
static int fav_batch_host(bls_ctx* ctx, const FavItems& h, uint8_t* out, const uint8_t* d_msgs = nullptr,
                          const uint8_t* d_keys = nullptr) {
  const size_t B = h.B;
  if (B > 0xffffffffull || (h.keys && h.keys->K > 0xffffffffull)) return BLS_E_ARG;
  if (h.msg_id) {  // before any device call
    if (!h.M) return BLS_E_ARG;
    for (size_t b = 0; b < B; b++)
      if (h.msg_id[b] >= h.M) return BLS_E_ARG;
  }
  const size_t nmsg = h.NH();
  FavItems it = h;  // the same batch over the device copies
  BitsArgs ba;
  uint32_t* d_idx;
  uint64_t* d_offs;
  uint8_t *d_m, *d_s, *d_out, *d_bits;
  if (h.bits) {
    SCR(S_IN0, h.bits->bytes, d_bits);
    CK(h2d(ctx, d_bits, h.bits->bits, h.bits->bytes));
    ba = BitsArgs{d_bits, h.bits->bytes, h.bits->mode};
    it.bits = &ba;
  } else {
    const uint64_t nidx = h.offs[B];
    if (nidx && !h.idx) return BLS_E_ARG;
    if (nidx > 0xffffffffull * 64) return BLS_E_ARG;
    for (size_t b = 0; b < B; b++)
      if (h.offs[b + 1] < h.offs[b]) return BLS_E_ARG;
    SCR(S_IN0, nidx, d_idx);
    SCR(S_OFFS, B + 1, d_offs);
    CK(h2d(ctx, d_idx, h.idx, nidx * 4));
    CK(h2d(ctx, d_offs, h.offs, (B + 1) * 8));
    it.idx = d_idx;
    it.offs = d_offs;
  }
  KeyTable kt{nullptr, 0, nullptr};
  if (h.keys) {
    const size_t K = h.keys->K;
    if (K && !h.keys->keys48 && !d_keys) return BLS_E_ARG;
    uint8_t* d_k = const_cast<uint8_t*>(d_keys);
    if (!d_k) {
      SCR(S_KEYS_IN, 48 * K, d_k);
      CK(h2d(ctx, d_k, h.keys->keys48, 48 * K));
    }
    kt = KeyTable{d_k, K, nullptr};
    if (h.keys->valid) SCR(S_KVALID, K, kt.valid);
    it.keys = &kt;
  }
  d_m = const_cast<uint8_t*>(d_msgs);
  if (!d_m) {
    SCR(S_IN1, 32 * nmsg, d_m);
    CK(h2d(ctx, d_m, h.msgs, 32 * nmsg));
  }
  SCR(S_IN2, 96 * B, d_s);
  SCR(S_IN3, B, d_out);
  CK(h2d(ctx, d_s, h.sigs, 96 * B));
  uint8_t seed[32];
  CK(host_seed(ctx, seed));
  it.msgs = d_m;
  it.sigs = d_s;
  it.seed32 = seed;
  // the inputs were just copied on stream1: the hash on stream2 forks after them, never from a bisection's EV_BIS
  // (an earlier call's, recorded before these copies; the hash would read the previous contents of S_IN1)
  ctx->j->bis_pending = false;
  Fp12* f;
  CK(fav_prepare(ctx, it, &f));
  int ok = run_final_check(ctx, f, 1, false);
  if (ok < 0) return ok;
  CK(fav_finish(ctx, ok, true, d_out));
  CK(d2h(ctx, out, d_out, B));
  if (kt.valid) CK(d2h(ctx, h.keys->valid, kt.valid, kt.K));  // each copy into caller memory is complete on return
  return 1;
}

int bls_fav_batch_indexed_shared(bls_ctx* ctx, const uint32_t* idx, const uint64_t* offsets, size_t B,
                                 const uint8_t* msgs32, size_t M, const uint32_t* msg_id, const uint8_t* sigs96,
                                 uint8_t* out) {
  API_ENTER(ctx);
  if ((!offsets || !msgs32 || !msg_id || !sigs96 || !out) && B) return BLS_E_ARG;
  if (!B) return 1;
  return fav_batch_host(ctx, FavItems{B, idx, offsets, nullptr, msgs32, M, msg_id, sigs96, nullptr}, out);
}

int bls_fav_batch_indexed(bls_ctx* ctx, const uint32_t* idx, const uint64_t* offsets, size_t B, const uint8_t* msgs32,
                          const uint8_t* sigs96, uint8_t* out) {
  API_ENTER(ctx);
  if ((!offsets || !msgs32 || !sigs96 || !out) && B) return BLS_E_ARG;
  if (!B) return 1;
  return fav_batch_host(ctx, FavItems{B, idx, offsets, nullptr, msgs32, 0, nullptr, sigs96, nullptr}, out);
}

static std::vector<uint64_t> identity_offsets(size_t B) {  // one key per item
  std::vector<uint64_t> offs(B + 1);
  for (size_t i = 0; i <= B; i++) offs[i] = i;
  return offs;
}

// Gossip firehose: B independent Verify calls with
// registry keys = B FastAggregateVerify calls of one key each, through the
// same RLC batch (one final exponentiation) and bisection path.
int bls_verify_batch_indexed(bls_ctx* ctx, const uint32_t* idx, size_t B, const uint8_t* msgs32, const uint8_t* sigs96,
                             uint8_t* out) {
  if (!idx && B) return BLS_E_ARG;
  return bls_fav_batch_indexed(ctx, idx, identity_offsets(B).data(), B, msgs32, sigs96, out);
}

int bls_verify_batch_indexed_shared(bls_ctx* ctx, const uint32_t* idx, size_t B, const uint8_t* msgs32, size_t M,
                                    const uint32_t* msg_id, const uint8_t* sigs96, uint8_t* out) {
  if (!idx && B) return BLS_E_ARG;
  return bls_fav_batch_indexed_shared(ctx, idx, identity_offsets(B).data(), B, msgs32, M, msg_id, sigs96, out);
}

// Key-table batches: the keys come as bytes with the batch, not from the registry.  B == 0 still judges the table
// when the caller asks for the verdicts.
int bls_fav_batch_keys(bls_ctx* ctx, const uint8_t* keys48, size_t K, const uint32_t* idx, const uint64_t* offsets,
                       size_t B, const uint8_t* msgs32, size_t M, const uint32_t* msg_id, const uint8_t* sigs96,
                       uint8_t* out, uint8_t* out_key_valid) {
  API_ENTER(ctx);
  if (K > 0xffffffffull || B > 0xffffffffull || (!keys48 && K)) return BLS_E_ARG;
  if ((!offsets || !msgs32 || !sigs96 || !out) && B) return BLS_E_ARG;
  if (!B) {
    if (out_key_valid && K) {
      uint8_t *d_k, *d_v;
      RegKey* tab;
      SCR(S_KEYS_IN, 48 * K, d_k);
      SCR(S_KVALID, K, d_v);
      SCR(S_KTAB, K, tab);
      CK(h2d(ctx, d_k, keys48, 48 * K));
      HIPCK(launch_key_table(ctx->j->stream, d_k, K, tab, d_v));
      CK(d2h(ctx, out_key_valid, d_v, K));
    }
    return 1;
  }
  const KeyTable kt{keys48, K, out_key_valid};
  return fav_batch_host(ctx, FavItems{B, idx, offsets, nullptr, msgs32, msg_id ? M : 0, msg_id, sigs96, nullptr, &kt},
                        out);
}

static std::vector<uint32_t> identity_indices(size_t B) {  // item b's key is table entry b
  std::vector<uint32_t> idx(B);
  for (size_t i = 0; i < B; i++) idx[i] = (uint32_t)i;
  return idx;
}

int bls_verify_batch_keys(bls_ctx* ctx, const uint8_t* keys48, size_t B, const uint8_t* msgs32, size_t M,
                          const uint32_t* msg_id, const uint8_t* sigs96, uint8_t* out) {
  if (B > 0xffffffffull) return BLS_E_ARG;
  return bls_fav_batch_keys(ctx, keys48, B, identity_indices(B).data(), identity_offsets(B).data(), B, msgs32, M,
                            msg_id, sigs96, out, nullptr);
}

// N deposit signatures: the signing roots on the device (k_deposit_roots) from the uploaded keys, credentials and
// amounts, then the keys batch of one key per item on the same job -- table = the N keys, idx = the identity,
// messages = the roots where the kernel left them.
int bls_deposits_verify(bls_ctx* ctx, const uint8_t* pubkeys48, const uint8_t* wc32, const uint64_t* amounts,
                        const uint8_t* sigs96, const uint8_t* domain32, size_t N, uint8_t* out, uint8_t* out_roots32) {
  API_ENTER(ctx);
  if (N > 0xffffffffull || ((!pubkeys48 || !wc32 || !amounts || !sigs96 || !domain32 || !out) && N)) return BLS_E_ARG;
  if (!N) return 1;
  uint8_t *d_k, *d_wc, *d_dom, *d_roots;
  uint64_t* d_amt;
  SCR(S_KEYS_IN, 48 * N, d_k);
  SCR(S_SZ_A, 32 * N, d_wc);
  SCR(S_SZ_B, N, d_amt);
  SCR(S_SZ_Z, 32, d_dom);
  SCR(S_IN1, 32 * N, d_roots);
  CK(h2d(ctx, d_k, pubkeys48, 48 * N));
  CK(h2d(ctx, d_wc, wc32, 32 * N));
  CK(h2d(ctx, d_amt, amounts, 8 * N));
  CK(h2d(ctx, d_dom, domain32, 32));
  HIPCK(launch_deposit_roots(ctx->j->stream, d_k, d_wc, d_amt, d_dom, N, d_roots));
  // synchronous: no copy into the caller's buffer is pending if the batch below returns an error
  if (out_roots32) CK(d2h(ctx, out_roots32, d_roots, 32 * N));
  const KeyTable kt{pubkeys48, N, nullptr};
  const std::vector<uint32_t> idx = identity_indices(N);
  const std::vector<uint64_t> offs = identity_offsets(N);
  return fav_batch_host(ctx, FavItems{N, idx.data(), offs.data(), nullptr, nullptr, 0, nullptr, sigs96, nullptr, &kt},
                        out, d_roots, d_k);
}

int bls_fav_batch_committee_bits(bls_ctx* ctx, const uint32_t* comm_ids, const uint64_t* comm_offs,
                                 const uint8_t* bits, const uint64_t* bit_offs, size_t B, const uint8_t* msgs32,
                                 size_t M, const uint32_t* msg_id, const uint8_t* sigs96, int mode, uint8_t* out) {
  API_ENTER(ctx);
  if ((!comm_offs || !bit_offs || !msgs32 || !sigs96 || !out) && B) return BLS_E_ARG;
  if (!B) return 1;
  CK(bits_plan(ctx, comm_ids, comm_offs, bit_offs, B, mode));
  if (bit_offs[B] && !bits) return BLS_E_ARG;
  static const uint8_t none = 0;  // a batch whose items all have no member still takes the bits route
  const BitsArgs ba{bits ? bits : &none, (size_t)bit_offs[B], mode};
  return fav_batch_host(ctx, FavItems{B, nullptr, nullptr, &ba, msgs32, M, msg_id, sigs96, nullptr}, out);
}

// The item records say what the gather added: read back and summed here, so the batch itself pays nothing for it.
int bls_last_gather_work(bls_ctx* ctx, uint64_t* points_added, uint64_t* complement_items) {
  API_ENTER(ctx);
  uint64_t pts = 0, ncompl = 0;
  if (ctx->work_job && ctx->work_job->bits_B) {
    Job& J = *ctx->work_job;
    std::vector<BitsItem> it(J.bits_B);
    HIPCK(hipMemcpyAsync(it.data(), J.bits_items, J.bits_B * sizeof(BitsItem), hipMemcpyDeviceToHost, J.stream));
    HIPCK(hipStreamSynchronize(J.stream));
    for (size_t b = 0; b < J.bits_B; b++) {
      pts += it[b].len;
      if (it[b].flags & BITS_F_COMPLEMENT) {
        pts += J.bits_tab[b + 1] - J.bits_tab[b];  // its committees' sums
        ncompl++;
      }
    }
  }
  if (points_added) *points_added = pts;
  if (complement_items) *complement_items = ncompl;
  return 0;
}

int bls_last_batch_work(bls_ctx* ctx, uint64_t* hashes, uint64_t* miller_pairs) {
  API_ENTER(ctx);
  if (hashes) *hashes = ctx->last_hashes;
  if (miller_pairs) *miller_pairs = ctx->last_pairs;
  return 0;
}
int bls_last_fallback_stats(bls_ctx* ctx, uint64_t* fe_checks, uint64_t* rounds) {
  API_ENTER(ctx);
  Job& J = *ctx->stats_job;
  if (J.bis_dev_checks) {
    uint32_t n = 0;
    HIPCK(hipMemcpyAsync(&n, J.bis_dev_checks, sizeof n, hipMemcpyDeviceToHost, J.stream));
    HIPCK(hipStreamSynchronize(J.stream));
    J.bis_checks = n;
    J.bis_dev_checks = nullptr;
  }
  if (fe_checks) *fe_checks = J.bis_checks;
  if (rounds) *rounds = J.bis_rounds;
  return 0;
}

// ---------------------------------------------- pipelined FAV batches --
__global__ void k_fp12_set_one(Fp12* f) {
  if (threadIdx.x || blockIdx.x) return;
  *f = fp12_one();
}

// The job's own check of the product f, on its stream: h_own[0] once EV_OWN has passed (wide: on k_fe_wide)
static int enqueue_own_check(bls_ctx* ctx, const Fp12* f, bool wide) {
  Job& J = *ctx->j;
  int* d_own;
  SCR(S_OWN, 1, d_own);
  if (wide)
    PROF(P_FINAL_EXP, launch_fe_wide(J.stream, f, 1, d_own));
  else
    PROF(P_FINAL_EXP, launch_final_check_wave(J.stream, f, 1, d_own));
  HIPCK(hipMemcpyAsync(J.h_own, d_own, sizeof(int), hipMemcpyDeviceToHost, J.stream));
  HIPCK(hipEventRecord(J.ev[EV_OWN], J.stream));
  J.own_pending = true;
  return 0;
}

// exchange: the job API with a communicator on the context (bls_fav_job_submit_dev) -- the all-gather and the
// combined check go on the device here and the job's own check is left for a failing combined check (read_own);
// otherwise (one GPU, or the host-exchange API bls_fav_batch_partial_dev) the own check is enqueued right behind the
// product.  B == 0 (a rank whose shard is empty) is allowed only with the exchange: its partial is the identity, so
// the rank still joins every all-gather and its peers never wait for it.
static int job_submit(bls_ctx* ctx, const FavItems& it, bool exchange) {
  exchange = exchange && ctx->comm;
  const size_t B = it.B;
  if (!it.seed32 || (B && ((!it.offs && !it.bits) || !it.msgs || !it.sigs)) || (!B && !exchange)) return BLS_E_ARG;
  Job& J = *ctx->j;
  Fp12* f;
  if (B) {
    CK(fav_prepare(ctx, it, &f));
  } else {
    SCR(S_FPART, 1, f);
    hipLaunchKernelGGL(k_fp12_set_one, dim3(1), dim3(64), 0, J.stream, f);
    HIPCK(hipGetLastError());
    J.fav_B = 0;
    J.fav_ready = true;
    J.comm_pending = false;
  }
  uint8_t* d_b;
  SCR(S_BYTES, 576, d_b);
  HIPCK(launch_fp12_to_bytes(J.stream, f, d_b));
  HIPCK(hipMemcpyAsync(J.h_partial, d_b, 576, hipMemcpyDeviceToHost, J.stream));
  HIPCK(hipEventRecord(J.ev[EV_PARTIAL], J.stream));
  J.partial_pending = true;
  if (exchange) {
    if (B) {
      // the own check runs only if the combined one fails, at any later time (read_own): it gets a copy of the
      // product in a slot of its own, right behind it in stream order.  S_FPART is rewritten by every per-call
      // product (AggregateVerify, AggregateVerify batches, the pairing checks) on job 0 meanwhile, and a passing
      // one there would make a failing shard keep every status
      Fp12* own_f;
      SCR(S_OWN_F, 1, own_f);
      HIPCK(hipMemcpyAsync(own_f, f, sizeof(Fp12), hipMemcpyDeviceToDevice, J.stream));
    }
    CK(enqueue_comm_check(ctx));
    J.own_pending = false;
    J.own_state = B ? -2 : 1;  // -2: computed on demand (read_own); an empty shard passes
    return 1;
  }
  // this job's own check, right behind its product on its stream: a single-GPU caller reads it with
  // bls_fav_job_check_own (no host round trip of the partial), and a multi-GPU failure is localised by it
  // knob BLS_FE_WIDE_MAX: the check of batches below that size on the six-wave k_fe_wide (0.65 ms against 1.13, six
  // waves against one): C3 -4.5 %, C5 unchanged (profiles/r06y_acc8_ab.txt), so off
  CK(enqueue_own_check(ctx, f, B < knobs().fe_wide_max));
  J.own_state = -1;
  return 1;
}

// The job-submit entry points' tail.  arg_error: what the entry point itself refused (0: submit).  With a
// communicator, a rank that fails here never enqueues the all-gather its peers are (or will be) in: abort, so their
// collectives fail instead of hanging (comm_fail_abort)
static int job_submit_exchange(bls_ctx* ctx, int arg_error, const FavItems& it) {
  const int r = arg_error ? arg_error : job_submit(ctx, it, true);
  if (r < 0 && ctx->comm) comm_fail_abort(ctx);
  return r;
}

// *state = the job's own verdict (1 / 0): waits for the check job_submit enqueued or, after a submit with the
// device exchange, runs it now (a failing combined check is the only reader).  Returns 0 or BLS_E_* (no verdict:
// no batch submitted on this job, or another batch prepared on the slot since).
static int read_own(bls_ctx* ctx, int* state) {
  Job& J = *ctx->j;
  if (J.own_state == -2) CK(enqueue_own_check(ctx, (const Fp12*)J.buf[S_OWN_F].p, false));
  if (J.own_pending) {
    HIPCK(hipEventSynchronize(J.ev[EV_OWN]));
    J.own_state = J.h_own[0] ? 1 : 0;
    J.own_pending = false;
  }
  if (J.own_state < 0) {
    ctx->err = "no submitted FAV batch on this job";
    return BLS_E_ARG;
  }
  *state = J.own_state;
  return 0;
}

static int job_partial(bls_ctx* ctx, uint8_t* partial576) {
  Job& J = *ctx->j;
  if (!partial576) return BLS_E_ARG;
  if (!J.partial_pending) {
    ctx->err = "no submitted FAV batch on this job";
    return BLS_E_ARG;
  }
  HIPCK(hipEventSynchronize(J.ev[EV_PARTIAL]));
  memcpy(partial576, J.h_partial, 576);
  J.partial_pending = false;
  return 1;
}

static int job_check(bls_ctx* ctx, const uint8_t* partials576, size_t n) {
  if (!partials576 || !n) return BLS_E_ARG;
  uint8_t* d_b;
  Fp12* f;
  SCR(S_IN0, 576 * n, d_b);
  SCR(S_FCHK, n, f);
  CK(h2d(ctx, d_b, partials576, 576 * n));
  PROF(P_PARTIALS_PROD, launch_fp12_from_bytes(ctx->j->stream, d_b, n, f));
  return run_final_check(ctx, f, (int)n, false);  // the n partials are multiplied inside the FE kernel
}

// Verdicts are written on the job's stream: a failing batch's bisection runs there without a host round trip, so
// the caller can check the next job meanwhile (bls_sync / bls_d2h wait for every job stream).
static int job_finish(bls_ctx* ctx, int batch_ok, uint8_t* d_out) {
  if (!d_out && ctx->j->fav_B) return BLS_E_ARG;
  bool root_bad = false;
  Job& J = *ctx->j;
  // a failed product of several shards (or of given partials): this job's own check decides.  Without a verdict
  // of its own (another batch was prepared on the slot since its submit) the bisection starts at the root, whose
  // check it runs first.
  if (!batch_ok && (J.own_pending || J.own_state != -1)) {
    int own = 0;
    CK(read_own(ctx, &own));
    if (own == 1) batch_ok = 1;  // its own product passes: the failure is elsewhere, every status stands
    else root_bad = true;        // its own product fails: bisect below the root
  }
  CK(fav_finish(ctx, batch_ok, root_bad, d_out));
  return 1;
}

int bls_fav_batch_partial_dev(bls_ctx* ctx, const uint32_t* d_idx, const uint64_t* d_offsets, size_t B,
                              const uint8_t* d_msgs32, const uint8_t* d_sigs96, const uint8_t* seed32,
                              uint8_t* partial576) {
  API_ENTER(ctx);
  if (!partial576) return BLS_E_ARG;
  const int r = job_submit(ctx, FavItems{B, d_idx, d_offsets, nullptr, d_msgs32, 0, nullptr, d_sigs96, seed32}, false);
  if (r < 0) return r;
  return job_partial(ctx, partial576);
}

int bls_partials_check(bls_ctx* ctx, const uint8_t* partials576, size_t n) {
  API_ENTER(ctx);
  return job_check(ctx, partials576, n);
}

int bls_fav_batch_finish_dev(bls_ctx* ctx, int batch_ok, uint8_t* d_out) {
  API_ENTER(ctx);
  return job_finish(ctx, batch_ok, d_out);
}

int bls_fav_job_submit_dev(bls_ctx* ctx, int job, const uint32_t* d_idx, const uint64_t* d_offsets, size_t B,
                           const uint8_t* d_msgs32, const uint8_t* d_sigs96, const uint8_t* seed32) {
  JOB_ENTER(ctx, job);
  return job_submit_exchange(ctx, 0, FavItems{B, d_idx, d_offsets, nullptr, d_msgs32, 0, nullptr, d_sigs96, seed32});
}

int bls_fav_job_submit_shared_dev(bls_ctx* ctx, int job, const uint32_t* d_idx, const uint64_t* d_offsets, size_t B,
                                  const uint8_t* d_msgs32, size_t M, const uint32_t* msg_id,
                                  const uint8_t* d_sigs96, const uint8_t* seed32) {
  JOB_ENTER(ctx, job);
  // an empty shard has no ids; fav_prepare refuses M == 0 and ids >= M before any device call
  const FavItems it{B, d_idx, d_offsets, nullptr, d_msgs32, M, B ? msg_id : nullptr, d_sigs96, seed32};
  return job_submit_exchange(ctx, (!B || msg_id) ? 0 : BLS_E_ARG, it);
}

// msg_id == nullptr: one message per item; else the shared-message form over a table of M.  An empty shard
// (B == 0, the device exchange only) takes no table and no bits.
int bls_fav_job_submit_bits_dev(bls_ctx* ctx, int job, const uint32_t* comm_ids, const uint64_t* comm_offs,
                                const uint8_t* d_bits, const uint64_t* bit_offs, size_t B, const uint8_t* d_msgs32,
                                size_t M, const uint32_t* msg_id, const uint8_t* d_sigs96, int mode,
                                const uint8_t* seed32) {
  JOB_ENTER(ctx, job);
  int r = B ? bits_plan(ctx, comm_ids, comm_offs, bit_offs, B, mode) : 0;
  if (r == 0 && B && bit_offs[B] && !d_bits) r = BLS_E_ARG;
  const BitsArgs ba{d_bits, 0, mode};
  return job_submit_exchange(ctx, r, FavItems{B, nullptr, nullptr, B ? &ba : nullptr, d_msgs32, msg_id ? M : 0,
                                              B ? msg_id : nullptr, d_sigs96, seed32});
}

// The key-table form: d_keys48 (K keys) device resident like the index lists; msg_id == nullptr: one message per
// item.  An empty shard (B == 0, the device exchange only) takes no table.
int bls_fav_job_submit_keys_dev(bls_ctx* ctx, int job, const uint8_t* d_keys48, size_t K, const uint32_t* d_idx,
                                const uint64_t* d_offsets, size_t B, const uint8_t* d_msgs32, size_t M,
                                const uint32_t* msg_id, const uint8_t* d_sigs96, const uint8_t* seed32) {
  JOB_ENTER(ctx, job);
  const int r = (K > 0xffffffffull || B > 0xffffffffull || (K && !d_keys48)) ? BLS_E_ARG : 0;
  const KeyTable kt{d_keys48, K, nullptr};
  FavItems it{B, d_idx, d_offsets, nullptr, d_msgs32, msg_id ? M : 0, B ? msg_id : nullptr, d_sigs96, seed32};
  if (B) it.keys = &kt;
  return job_submit_exchange(ctx, r, it);
}

int bls_fav_job_partial(bls_ctx* ctx, int job, uint8_t* partial576) {
  JOB_ENTER(ctx, job);
  return job_partial(ctx, partial576);
}

int bls_fav_job_check(bls_ctx* ctx, int job, const uint8_t* partials576, size_t n) {
  JOB_ENTER(ctx, job);
  return job_check(ctx, partials576, n);
}

int bls_fav_job_check_own(bls_ctx* ctx, int job) {
  JOB_ENTER(ctx, job);
  int own = 0;
  CK(read_own(ctx, &own));
  ctx->j->partial_pending = false;  // the partial's host copy is not needed
  return own;
}

int bls_fav_job_finish_dev(bls_ctx* ctx, int job, int batch_ok, uint8_t* d_out) {
  JOB_ENTER(ctx, job);
  return job_finish(ctx, batch_ok, d_out);
}

}  // extern "C"
