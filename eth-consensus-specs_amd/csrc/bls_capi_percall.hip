// C ABI, the per-call signature API (Verify, FastAggregateVerify, AggregateVerify and its batch, Aggregate, Sign,
// SkToPk, hash_to_G2).
#include "bls_capi_internal.h"

namespace {

__global__ void k_copy_int(const int* src, int* dst) {
  if (threadIdx.x == 0) *dst = *src;
}

__global__ void k_set_neg_g1(G1A* p) {
  if (threadIdx.x || blockIdx.x) return;
  G1A g = g1_generator();
  g.y = fp_neg(g.y);
  *p = g;
}

__global__ void k_set_fp2_one(Fp2* z) {
  if (threadIdx.x || blockIdx.x) return;
  *z = fp2_one();
}

}  // namespace

extern "C" {

// Per-call CoreVerify over n keys (n = 1: Verify, E/utils/bls.py:141-151;
// n > 1: FastAggregateVerify, :167-177), on three streams, in wavefront-cooperative arithmetic:
//   stream2: hash_to_G2(msg) on one wave (k_h2c_wide)
//   stream3 (job 0's third stream, or the context's per-call stream when job 0 has two): signature decode + G2
//            subgroup check (k_sig_validate_wide)
//            then the Miller loop of (-G1, sigma) on one k_miller_wide workgroup (it overlaps the hash's tail)
//   stream1: KeyValidate of every key (+ their sum), then -- after the hash --
//            the Miller loop of (apk, H) on another, the six-wave final
//            exponentiation (k_fe_wide) of both loops' product on the same
//            stream, and both verdict words (FE, live) back in one pinned copy.
static int verify_percall(bls_ctx* ctx, const uint8_t* pks48, size_t n, const uint8_t* msg, size_t msg_len,
                          const uint8_t* sig96) {
  Job& J = *ctx->j;
  hipStream_t st = J.stream, st2 = J.stream2, st3 = J.stream3;
  uint8_t* d_in;
  G1A *keys, *P;
  G2A* Q;
  int *ok, *d_r;
  G1J *tmp, *apk;
  int* flag;
  Fp12* f;
  uint64_t* d_offs;
  const size_t in_bytes = 48 * n + 96 + msg_len;
  const size_t offs_at = (in_bytes + 7) & ~(size_t)7;  // the two message offsets after the inputs, 8-B aligned
  const size_t total = offs_at + 16;
  SCR(S_IN0, total, d_in);
  d_offs = reinterpret_cast<uint64_t*>(d_in + offs_at);
  SCR(S_G1A, n, keys);
  SCR(S_OK, n + 2, ok);  // key verdicts | sig verdict | live
  SCR(S_PC_P, 3, P);  // P[0] apk, P[1] -G1 (k_percall_pairs), P[2] -G1 (the signature's pair, its own stream)
  SCR(S_G2A, 2, Q);
  Fp2* hz = nullptr;  // H's Jacobian Z (k_h2c_wide skips its inversion; the Miller loop's additions take Q as is)
  if (!ctx->force_fb) SCR(S_G2A_B, 1, hz);  // (the forced-fallback test hook overwrites H affine after the kernel)
  Fp* pz = nullptr;  // the key sum's Jacobian Z (no inversion; the Miller loop scales its lines by Z^3)
  if (n > 1) SCR(S_PC_PZ, 1, pz);
  SCR(S_G1J_T, 1024, tmp);
  SCR(S_G1J, 1, apk);
  SCR(S_AV_FLAG, 1, flag);
  SCR(S_F, 2, f);  // f(apk, H) | f(-G1, sigma)
  SCR(S_INT, 4, d_r);
  uint8_t* d_pk = d_in;
  uint8_t* d_sig = d_in + 48 * n;
  uint8_t* d_msg = d_in + 48 * n + 96;
  const uint64_t offs[2] = {0, msg_len};
  if (ctx->pc_stage_cap < total) {  // grows to the largest call seen; the previous call has synchronised
    if (ctx->pc_stage) HIPCK(hipHostFree(ctx->pc_stage));
    ctx->pc_stage = nullptr;
    ctx->pc_stage_cap = 0;
    HIPCK(hipHostMalloc((void**)&ctx->pc_stage, total, hipHostMallocDefault));
    ctx->pc_stage_cap = total;
  }
  memcpy(ctx->pc_stage, pks48, 48 * n);
  memcpy(ctx->pc_stage + 48 * n, sig96, 96);
  if (msg_len) memcpy(ctx->pc_stage + 48 * n + 96, msg, msg_len);
  memcpy(ctx->pc_stage + offs_at, offs, sizeof offs);
  CK(h2d(ctx, d_in, ctx->pc_stage, total));
  // a two-stream job 0 (stream3 aliases stream2): the signature check on the context's per-call stream, beside
  // the hash and the keys (on stream1 ahead of the keys it made stream1 as long as the hash: 0.8 + 0.7 ms)
  const hipStream_t ss = st3 != st2 ? st3 : ctx->pc_stream;
  HIPCK(hipEventRecord(J.ev[EV_FORK], st));
  HIPCK(hipStreamWaitEvent(st2, J.ev[EV_FORK], 0));
  if (ss != st) HIPCK(hipStreamWaitEvent(ss, J.ev[EV_FORK], 0));
  // one wave of wavefront-cooperative arithmetic for the one message (bls_wide.h); 32-byte messages (every
  // signing root) take the register-resident expand_message_xmd
  const uint64_t* h_offs = msg_len == 32 ? nullptr : d_offs;
  HIPCK(launch_h2c_wide(st2, 1, d_msg, h_offs, Q, flag, hz));
  CK(h2c_fallback(ctx, st2, 1, d_msg, h_offs, flag, Q));
  HIPCK(hipEventRecord(J.ev[EV_JOIN], st2));
  HIPCK(launch_sig_validate_wide(ss, d_sig, 1, Q + 1, ok + n));
  HIPCK(hipEventRecord(J.ev[EV_SIG], ss));
  // (-G1, sigma)'s Miller loop right behind the signature check, beside the hash (constant lines for a rejected
  // signature): one pair per workgroup, so the critical path after the hash is one pair's loop, not two
  hipLaunchKernelGGL(k_set_neg_g1, dim3(1), dim3(64), 0, ss, P + 2);
  HIPCK(hipGetLastError());
  HIPCK(launch_miller_wide(ss, P + 2, Q + 1, ok + n, nullptr, 1, f + 1));
  HIPCK(hipEventRecord(J.ev[EV_MSM], ss));
  HIPCK(launch_keys(st, d_pk, n, keys, ok));
  if (n > 1) HIPCK(launch_g1_sum_aff(st, keys, nullptr, n, tmp, apk));
  HIPCK(hipStreamWaitEvent(st, J.ev[EV_SIG], 0));
  HIPCK(launch_percall_pairs(st, keys, ok, n, apk, ok + n, P, ok + n + 1, pz));
  HIPCK(hipStreamWaitEvent(st, J.ev[EV_JOIN], 0));
  // (apk, H): rejected inputs are identities there, `live` decides
  HIPCK(launch_miller_wide(st, P, Q, nullptr, nullptr, 1, f, hz, pz));
  HIPCK(hipStreamWaitEvent(st, J.ev[EV_MSM], 0));
  // the six-wave final check of f(apk, H) f(-G1, sigma) on the same stream, then both verdict words in one copy
  // (FE | live) and one sync
  PROF2(P_FINAL_EXP, st, launch_fe_wide(st, f, 2, d_r));
  hipLaunchKernelGGL(k_copy_int, dim3(1), dim3(64), 0, st, ok + n + 1, d_r + 1);
  HIPCK(hipGetLastError());
  int res[2] = {0, 0};
  HIPCK(hipMemcpyAsync(ctx->pc_stage, d_r, sizeof res, hipMemcpyDeviceToHost, st));
  HIPCK(hipStreamSynchronize(st));
  memcpy(res, ctx->pc_stage, sizeof res);
  return (res[0] && res[1]) ? 1 : 0;
}

int bls_verify(bls_ctx* ctx, const uint8_t* pk48, const uint8_t* msg, size_t msg_len, const uint8_t* sig96) {
  API_ENTER(ctx);
  if (!pk48 || !sig96 || (!msg && msg_len) || msg_len > 0xffffffffu) return BLS_E_ARG;
  return verify_percall(ctx, pk48, 1, msg, msg_len, sig96);
}

int bls_fast_aggregate_verify(bls_ctx* ctx, const uint8_t* pks48, size_t n, const uint8_t* msg, size_t msg_len,
                              const uint8_t* sig96) {
  API_ENTER(ctx);
  if ((!pks48 && n) || !sig96 || (!msg && msg_len) || msg_len > 0xffffffffu) return BLS_E_ARG;
  if (n == 0) return 0;
  return verify_percall(ctx, pks48, n, msg, msg_len, sig96);
}

int bls_aggregate_verify(bls_ctx* ctx, const uint8_t* pks48, size_t n, const uint8_t* msgs, const size_t* msg_lens,
                         const uint8_t* sig96) {
  API_ENTER(ctx);
  if ((!pks48 || !msg_lens) && n) return BLS_E_ARG;
  if (!sig96) return BLS_E_ARG;
  if (n == 0) return 0;
  std::vector<uint64_t> offs(n + 1, 0);
  for (size_t i = 0; i < n; i++) {
    if (msg_lens[i] > 0xffffffffu) return BLS_E_ARG;
    offs[i + 1] = offs[i] + msg_lens[i];
  }
  if (offs[n] && !msgs) return BLS_E_ARG;
  // three streams as verify_percall: the signature's decode + subgroup check (stream3) and the n hashes
  // (stream2) run beside the keys' validation (stream1, which synchronises for the verdicts), the Miller loops
  // join them; a rejected signature is reported through its verdict word next to the FE result
  Job& J = *ctx->j;
  hipStream_t st = J.stream, st2 = J.stream2, st3 = J.stream3;
  uint8_t *d_sig, *d_msgs;
  uint64_t* d_offs;
  G2A* Q;
  int* d_w;
  Fp12 *f, *ft, *fo;
  Fd* d_hf;
  int* d_flag;
  SCR(S_IN1, 96, d_sig);
  SCR(S_IN2, offs[n], d_msgs);
  SCR(S_OFFS, n + 1, d_offs);
  SCR(S_G2A, n + 1, Q);
  SCR(S_INT, 4, d_w);  // sig verdict | FE verdict
  SCR(S_F, n + 1, f);
  SCR(S_F_T, (n + 1) / 8 + 16, ft);
  SCR(S_FPART, 1, fo);
  SCR(S_AV_HCF, h2c_scratch_fd(n), d_hf);
  SCR(S_AV_FLAG, n, d_flag);
  // the hashes in Jacobian coordinates when both the hash and the Miller loop take the wide kernels (no inversion
  // per message; Z of the signature's pair 1); not under the forced-fallback test hook (it rewrites H affine)
  Fp2* hz = nullptr;
  const size_t wide_h2c_max = knobs().wide_h2c_max;
  if (n <= wide_h2c_max && n + 1 <= knobs().wide_miller_max && !ctx->force_fb) SCR(S_G2A_B, n + 1, hz);
  CK(h2d(ctx, d_sig, sig96, 96));
  CK(h2d(ctx, d_msgs, msgs, offs[n]));
  CK(h2d(ctx, d_offs, offs.data(), (n + 1) * sizeof(uint64_t)));
  const hipStream_t ss = st3 != st2 ? st3 : ctx->pc_stream;  // two-stream job 0: the per-call stream (verify_percall)
  HIPCK(hipEventRecord(J.ev[EV_FORK], st));
  HIPCK(hipStreamWaitEvent(st2, J.ev[EV_FORK], 0));
  if (ss != st) HIPCK(hipStreamWaitEvent(ss, J.ev[EV_FORK], 0));
  HIPCK(launch_sig_validate_wide(ss, d_sig, 1, Q + n, d_w));
  if (hz) {
    hipLaunchKernelGGL(k_set_fp2_one, dim3(1), dim3(64), 0, ss, hz + n);
    HIPCK(hipGetLastError());
  }
  HIPCK(hipEventRecord(J.ev[EV_SIG], ss));
  bool m32 = true;  // all signing roots: the FAV batches' 32-byte h2c kernels (msgs are then 32 B apart)
  for (size_t i = 0; i < n && m32; i++) m32 = msg_lens[i] == 32;
  // up to ~a thousand messages one wide workgroup each, lower latency than the lane chains (tools/av_probe.py: 1,024
  // messages 7.95 -> 6.85 ms; 8,192 took 15.1 -> 31.5 ms, past the chip's CUs); knob BLS_WIDE_H2C_MAX
  if (n <= wide_h2c_max)
    HIPCK(launch_h2c_wide(st2, n, d_msgs, m32 ? nullptr : d_offs, Q, d_flag, hz));
  else if (m32)
    HIPCK(launch_h2c(st2, n, d_msgs, nullptr, d_hf, Q, d_flag));
  else
    HIPCK(launch_h2c_msgs(st2, n, d_msgs, d_offs, d_hf, Q, d_flag));
  CK(h2c_fallback(ctx, st2, n, d_msgs, m32 ? nullptr : d_offs, d_flag, Q));
  HIPCK(hipEventRecord(J.ev[EV_JOIN], st2));
  G1A* P;
  int* ok;
  const int v = validate_pks(ctx, pks48, n, &P, &ok);  // synchronises stream1
  if (v <= 0) {
    HIPCK(hipStreamSynchronize(st2));  // the scratch of the side streams is reused by the next call
    HIPCK(hipStreamSynchronize(ss));
    return v;
  }
  HIPCK(hipStreamWaitEvent(st, J.ev[EV_SIG], 0));
  HIPCK(hipStreamWaitEvent(st, J.ev[EV_JOIN], 0));
  hipLaunchKernelGGL(k_set_neg_g1, dim3(1), dim3(64), 0, st, P + n);
  HIPCK(hipGetLastError());
  size_t nf = 0;
  HIPCK(launch_miller_call(st, P, Q, n + 1, f, &nf, hz));  // a rejected signature: constant lines there
  HIPCK(launch_fp12_prod_vm(st, f, nf, ft, fo));
  PROF2(P_FINAL_EXP, st, launch_fe_wide(st, fo, 1, d_w + 1));
  int w[2] = {0, 0};
  CK(d2h(ctx, w, d_w, sizeof w));
  return (w[0] && w[1]) ? 1 : 0;
}

int bls_aggregate(bls_ctx* ctx, const uint8_t* sigs96, size_t n, uint8_t* out96) {
  API_ENTER(ctx);
  if ((!sigs96 && n) || !out96) return BLS_E_ARG;
  if (n == 0) return 0;
  uint8_t *d_in, *d_out;
  G2A* a;
  int* d_ok;
  G2J *tmp, *s;
  SCR(S_IN0, 96 * n, d_in);
  SCR(S_G2A, n, a);
  SCR(S_OK, n, d_ok);
  SCR(S_G2J_T, 1024, tmp);
  SCR(S_G2J, 1, s);
  SCR(S_IN1, 96, d_out);
  CK(h2d(ctx, d_in, sigs96, 96 * n));
  HIPCK(launch_sig_validate(ctx->j->stream, d_in, n, a, d_ok));
  const int v = all_ok(ctx, d_ok, n);
  if (v <= 0) return v;
  HIPCK(launch_g2_sum_aff(ctx->j->stream, a, nullptr, n, tmp, s));
  HIPCK(launch_g2_compress(ctx->j->stream, s, d_out));
  CK(d2h(ctx, out96, d_out, 96));
  return 1;
}

int bls_aggregate_pks(bls_ctx* ctx, const uint8_t* pks48, size_t n, uint8_t* out48) {
  API_ENTER(ctx);
  if ((!pks48 && n) || !out48) return BLS_E_ARG;
  if (n == 0) return 0;
  G1A* a;
  int* ok;
  int v = validate_pks(ctx, pks48, n, &a, &ok);
  if (v <= 0) return v;
  G1J *tmp, *s;
  uint8_t* d_out;
  SCR(S_G1J_T, 1024, tmp);
  SCR(S_G1J, 1, s);
  SCR(S_IN1, 48, d_out);
  HIPCK(launch_g1_sum_aff(ctx->j->stream, a, nullptr, n, tmp, s));
  HIPCK(launch_g1_compress(ctx->j->stream, s, d_out, nullptr));
  CK(d2h(ctx, out48, d_out, 48));
  return 1;
}

int bls_key_validate(bls_ctx* ctx, const uint8_t* pk48) {
  API_ENTER(ctx);
  if (!pk48) return BLS_E_ARG;
  G1A* a;
  int* ok;
  return validate_pks(ctx, pk48, 1, &a, &ok);
}

static int sign_impl(bls_ctx* ctx, const uint8_t* sks, const uint8_t* msgs, const uint64_t* offs, size_t n,
                     uint8_t* out96) {
  uint8_t *d_sk, *d_m, *d_out;
  uint64_t* d_offs;
  int* d_ok;
  SCR(S_IN0, 32 * n, d_sk);
  SCR(S_IN1, offs[n], d_m);
  SCR(S_IN2, 96 * n, d_out);
  SCR(S_OFFS, n + 1, d_offs);
  SCR(S_OK, n, d_ok);
  CK(h2d(ctx, d_sk, sks, 32 * n));
  CK(h2d(ctx, d_m, msgs, offs[n]));
  CK(h2d(ctx, d_offs, offs, (n + 1) * sizeof(uint64_t)));
  HIPCK(launch_sign_many(ctx->j->stream, d_sk, d_m, d_offs, n, d_out, d_ok));
  const int v = all_ok(ctx, d_ok, n);
  if (v < 0) return v;
  CK(d2h(ctx, out96, d_out, 96 * n));
  return v;
}

int bls_sign(bls_ctx* ctx, const uint8_t* sk32, const uint8_t* msg, size_t msg_len, uint8_t* out96) {
  API_ENTER(ctx);
  if (!sk32 || !out96 || (!msg && msg_len) || msg_len > 0xffffffffu) return BLS_E_ARG;
  uint64_t offs[2] = {0, msg_len};
  return sign_impl(ctx, sk32, msg, offs, 1, out96);
}

int bls_sign_batch(bls_ctx* ctx, const uint8_t* sks32, const uint8_t* msgs32, size_t B, uint8_t* out96) {
  API_ENTER(ctx);
  if ((!sks32 || !msgs32 || !out96) && B) return BLS_E_ARG;
  if (!B) return 1;
  std::vector<uint64_t> offs(B + 1);
  for (size_t i = 0; i <= B; i++) offs[i] = 32 * i;
  return sign_impl(ctx, sks32, msgs32, offs.data(), B, out96);
}

static int sk_to_pk_impl(bls_ctx* ctx, const uint8_t* sks, size_t n, uint8_t* out48) {
  uint8_t *d_sk, *d_out;
  int* d_ok;
  SCR(S_IN0, 32 * n, d_sk);
  SCR(S_IN2, 48 * n, d_out);
  SCR(S_OK, n, d_ok);
  CK(h2d(ctx, d_sk, sks, 32 * n));
  HIPCK(launch_sk_to_pk_many(ctx->j->stream, d_sk, n, d_out, d_ok));
  const int v = all_ok(ctx, d_ok, n);
  if (v < 0) return v;
  CK(d2h(ctx, out48, d_out, 48 * n));
  return v;
}

int bls_sk_to_pk(bls_ctx* ctx, const uint8_t* sk32, uint8_t* out48) {
  API_ENTER(ctx);
  if (!sk32 || !out48) return BLS_E_ARG;
  return sk_to_pk_impl(ctx, sk32, 1, out48);
}

int bls_sk_to_pk_batch(bls_ctx* ctx, const uint8_t* sks32, size_t B, uint8_t* out48) {
  API_ENTER(ctx);
  if ((!sks32 || !out48) && B) return BLS_E_ARG;
  if (!B) return 1;
  return sk_to_pk_impl(ctx, sks32, B, out48);
}

int bls_hash_to_g2(bls_ctx* ctx, const uint8_t* msg, size_t msg_len, const uint8_t* dst, size_t dst_len,
                   uint8_t* out96) {
  API_ENTER(ctx);
  if (!out96 || (!msg && msg_len) || !dst || dst_len == 0 || dst_len > 255 || msg_len > 0xffffffffu) return BLS_E_ARG;
  uint8_t *d_m, *d_dst, *d_out;
  uint64_t* d_offs;
  G2A* h;
  SCR(S_IN0, msg_len, d_m);
  SCR(S_IN1, dst_len, d_dst);
  SCR(S_IN2, 96, d_out);
  SCR(S_OFFS, 2, d_offs);
  SCR(S_G2A, 1, h);
  uint64_t offs[2] = {0, msg_len};
  CK(h2d(ctx, d_m, msg, msg_len));
  CK(h2d(ctx, d_dst, dst, dst_len));
  CK(h2d(ctx, d_offs, offs, sizeof offs));
  HIPCK(launch_hash_many(ctx->j->stream, d_m, d_offs, 1, d_dst, (uint32_t)dst_len, h));
  HIPCK(launch_g2_compress_aff(ctx->j->stream, h, d_out));
  CK(d2h(ctx, out96, d_out, 96));
  return 1;
}
int bls_aggregate_verify_batch(bls_ctx* ctx, const uint8_t* pks48, const uint8_t* msgs, const uint64_t* msg_offs,
                               const uint64_t* item_offs, size_t B, const uint8_t* sigs96, uint8_t* out) {
  API_ENTER(ctx);
  if ((B && (!item_offs || !sigs96 || !out)) || B > 0xffffffffu) return BLS_E_ARG;
  if (B == 0) return 1;
  if (item_offs[0] != 0) return BLS_E_ARG;
  for (size_t b = 0; b < B; b++)
    if (item_offs[b + 1] < item_offs[b]) return BLS_E_ARG;
  const size_t total = item_offs[B];
  if (total && (!pks48 || !msg_offs)) return BLS_E_ARG;
  if (total > 0xffffffffu) return BLS_E_ARG;
  if (total) {
    if (msg_offs[0] != 0) return BLS_E_ARG;
    for (size_t t = 0; t < total; t++)
      if (msg_offs[t + 1] < msg_offs[t] || msg_offs[t + 1] - msg_offs[t] > 0xffffffffu) return BLS_E_ARG;
    if (msg_offs[total] && !msgs) return BLS_E_ARG;
  }
  ctx->j->bis_checks = ctx->j->bis_rounds = 0;
  ctx->j->bis_dev_checks = nullptr;
  ctx->stats_job = ctx->j;
  hipStream_t st = ctx->j->stream;
  const size_t npair = total + B;
  // inputs
  uint8_t *d_pk, *d_sig, *d_msgs;
  uint64_t *d_moffs, *d_io, *d_rsc;
  uint32_t* d_pitem;
  SCR(S_IN0, 48 * total, d_pk);
  SCR(S_IN1, 96 * B, d_sig);
  SCR(S_IN2, total ? msg_offs[total] : 0, d_msgs);
  SCR(S_OFFS, total + 1, d_moffs);
  SCR(S_AV_IO, B + 1, d_io);
  SCR(S_AV_RSC, B, d_rsc);
  SCR(S_AV_PITEM, total, d_pitem);
  std::vector<uint32_t> pitem(total);
  for (size_t b = 0; b < B; b++)
    for (uint64_t t = item_offs[b]; t < item_offs[b + 1]; t++) pitem[t] = (uint32_t)b;
  std::vector<uint64_t> rsc(B);
  {
    uint8_t seed[32];
    CK(host_seed(ctx, seed));
    uint64_t x = 0, y = 0;
    memcpy(&x, seed, 8);
    memcpy(&y, seed + 8, 8);
    for (size_t b = 0; b < B; b++) {  // splitmix64 stream keyed by the OS seed; r_b != 0
      x += 0x9e3779b97f4a7c15ull;
      uint64_t z = x ^ y;
      z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
      z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
      z ^= z >> 31;
      rsc[b] = z ? z : 1;
    }
  }
  CK(h2d(ctx, d_pk, pks48, 48 * total));
  CK(h2d(ctx, d_sig, sigs96, 96 * B));
  if (total) {
    CK(h2d(ctx, d_msgs, msgs, msg_offs[total]));
    CK(h2d(ctx, d_moffs, msg_offs, (total + 1) * sizeof(uint64_t)));
  }
  CK(h2d(ctx, d_io, item_offs, (B + 1) * sizeof(uint64_t)));
  CK(h2d(ctx, d_rsc, rsc.data(), B * sizeof(uint64_t)));
  CK(h2d(ctx, d_pitem, pitem.data(), total * sizeof(uint32_t)));
  // per-key / per-signature validation, hash_to_G2 of every message
  G1A *d_pa, *P2;
  G2A *d_sa, *d_h, *Q2;
  int *d_pok, *d_sok, *d_status, *d_res;
  Fp12 *f, *ft, *fo, *fi;
  SCR(S_G1A, total, d_pa);
  SCR(S_OK, total, d_pok);
  SCR(S_AV_SIG, B, d_sa);
  SCR(S_AV_SOK, B, d_sok);
  SCR(S_AV_H, total, d_h);
  SCR(S_AV_ST, B, d_status);
  SCR(S_AV_P, npair, P2);
  SCR(S_AV_Q, npair, Q2);
  SCR(S_AV_F, npair, f);
  SCR(S_AV_FT, npair / 8 + 16, ft);
  SCR(S_FPART, 1, fo);
  HIPCK(launch_key_validate(st, d_pk, total, d_pa, d_pok));
  HIPCK(launch_sig_validate(st, d_sig, B, d_sa, d_sok));
  {  // hash_to_G2 of every message (as in the FAV batch)
    Fd* d_hf;
    int* d_flag;
    SCR(S_AV_HCF, h2c_scratch_fd(total), d_hf);
    SCR(S_AV_FLAG, total, d_flag);
    HIPCK(launch_h2c_msgs(st, total, d_msgs, d_moffs, d_hf, d_h, d_flag));
    CK(h2c_fallback(ctx, st, total, d_msgs, d_moffs, d_flag, d_h));
  }
  HIPCK(launch_av_items(st, B, d_io, d_pok, d_sok, d_sa, d_rsc, d_status, P2, Q2));
  HIPCK(launch_av_pairs(st, total, d_pitem, d_status, d_rsc, d_pa, d_h, P2, Q2));
  if (npair >= 256) {  // per-pair Miller values (the fallback multiplies each item's segment): the fused kernel
                       // (G2 lines and f accumulation in one workgroup, bls_miller_pair.hip, G = 1)
    PROF(P_MILLER, launch_miller_fused(st, P2, Q2, nullptr, npair, f, 1));
  } else {
    PROF(P_MILLER, launch_miller_wave(st, P2, Q2, nullptr, npair, f));
  }
  PROF(P_FP12_PROD, launch_fp12_prod_vm(st, f, npair, ft, fo));
  std::vector<int> status(B);
  CK(d2h(ctx, status.data(), d_status, B * sizeof(int)));
  const int batch_ok = run_final_check(ctx, fo, 1, false);
  if (batch_ok < 0) return batch_ok;
  if (!batch_ok) {  // each item on its own: its segment of Miller values, one final exponentiation each
    std::vector<uint32_t> sel;
    for (size_t b = 0; b < B; b++)
      if (status[b]) sel.push_back((uint32_t)b);
    uint32_t* d_sel;
    SCR(S_AV_SEL, sel.size(), d_sel);
    SCR(S_AV_FI, B, fi);
    SCR(S_AV_RES, sel.size(), d_res);
    HIPCK(launch_fp12_seg_prod(st, f, d_io, B, fi));
    std::vector<int> res(sel.size());
    CK(run_final_checks_sel(ctx, fi, sel.data(), sel.size(), d_sel, d_res, res.data()));
    for (size_t k = 0; k < sel.size(); k++) status[sel[k]] = res[k];
    ctx->j->bis_checks = sel.size();
    ctx->j->bis_rounds = 1;
  }
  for (size_t b = 0; b < B; b++) out[b] = status[b] ? 1 : 0;
  return 1;
}

}  // extern "C"
