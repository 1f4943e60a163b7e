// C ABI, the multi-GPU exchange (RCCL).
// every rank reduces its shard to one 576-byte Fp12 Miller
// partial; ncclAllGather moves the world x 576 bytes over xGMI (the transfer
// is latency-bound, not bandwidth-bound), and every rank multiplies the
// partials inside its final-exponentiation kernel -- no broadcast.  Fp12
// multiplication is not an elementwise sum, so this is an all-gather, not an
// all-reduce.
#include "bls_capi_internal.h"

static int comm_abort_locked(bls_ctx* ctx) {
  if (ctx->comm) {
    (void)ncclCommAbort(ctx->comm);
    ctx->comm = nullptr;
  }
  ctx->comm_rank = 0;
  ctx->comm_world = 1;
  return 0;
}

namespace capi {

int nccl_fail(bls_ctx* c, ncclResult_t r, const char* where) {
  char b[256];
  snprintf(b, sizeof b, "%s: %s", where, ncclGetErrorString(r));
  c->err = b;
  return BLS_E_DEVICE;
}

// any error on the exchange path -- a local one included (this rank then skips an all-gather its peers are in)
// -- leaves the peers waiting in this or a later all-gather: abort so their collectives fail instead of hanging.
// The first failure's text stays in ctx->err and is repeated by every later call on this context.
void comm_fail_abort(bls_ctx* ctx) {
  ctx->comm_abort_cause = ctx->err;
  comm_abort_locked(ctx);
  ctx->err = "RCCL communicator aborted: " + ctx->comm_abort_cause;
}

// The device-side exchange of a submitted job (multi-GPU, a communicator on the context), enqueued at submit: the
// comm stream waits for the partial, all-gathers the world's 576-byte partials (the collectives of all jobs on one
// stream, in submission order -- every rank submits the same jobs in the same order, so the collectives match),
// and the job's stream multiplies them inside the final-exponentiation kernel and copies the 4-byte verdict to
// h_own[1] (EV_CV).  No host step between a job's product and its verdict.
int enqueue_comm_check(bls_ctx* ctx) {
  Job& J = *ctx->j;
  const int W = ctx->comm_world;
  uint8_t* d_all;
  Fp12* fw;
  int* d_cv;
  SCR(S_COMM, 576 * (size_t)W, d_all);
  SCR(S_FCHK, W, fw);
  SCR(S_CV, 1, d_cv);
  HIPCK(hipStreamWaitEvent(ctx->comm_stream, J.ev[EV_PARTIAL], 0));
  const ncclResult_t r = ncclAllGather(J.buf[S_BYTES].p, d_all, 576, ncclUint8, ctx->comm, ctx->comm_stream);
  if (r != ncclSuccess) return nccl_fail(ctx, r, "ncclAllGather");
  HIPCK(hipEventRecord(J.ev[EV_COMM], ctx->comm_stream));
  HIPCK(hipStreamWaitEvent(J.stream, J.ev[EV_COMM], 0));
  PROF(P_PARTIALS_PROD, launch_fp12_from_bytes(J.stream, d_all, W, fw));
  PROF(P_FINAL_EXP, launch_final_check_wave(J.stream, fw, W, d_cv));
  HIPCK(hipMemcpyAsync(J.h_own + 1, d_cv, sizeof(int), hipMemcpyDeviceToHost, J.stream));
  HIPCK(hipEventRecord(J.ev[EV_CV], J.stream));
  J.comm_pending = true;
  return 0;
}

}  // namespace capi

extern "C" {

int bls_comm_unique_id(uint8_t* out128) {
  if (!out128) return BLS_E_ARG;
  ncclUniqueId id;
  if (ncclGetUniqueId(&id) != ncclSuccess) return BLS_E_DEVICE;
  static_assert(sizeof(id) == 128, "ncclUniqueId is 128 bytes");
  memcpy(out128, &id, sizeof id);
  return 0;
}

int bls_comm_init(bls_ctx* ctx, const uint8_t* uid128, int rank, int world) {
  API_ENTER(ctx);
  if (!uid128 || world < 1 || rank < 0 || rank >= world) return BLS_E_ARG;
  if (ctx->comm) {
    (void)ncclCommDestroy(ctx->comm);
    ctx->comm = nullptr;
  }
  ncclUniqueId id;
  memcpy(&id, uid128, sizeof id);
  const ncclResult_t r = ncclCommInitRank(&ctx->comm, world, id, rank);
  if (r != ncclSuccess) {
    ctx->comm = nullptr;
    return nccl_fail(ctx, r, "ncclCommInitRank");
  }
  ctx->comm_rank = rank;
  ctx->comm_world = world;
  ctx->comm_abort_cause.clear();
  return 0;
}

int bls_comm_destroy(bls_ctx* ctx) {
  API_ENTER(ctx);
  if (ctx->comm) {
    HIPCK(hipStreamSynchronize(ctx->comm_stream));  // every all-gather enqueued by a submit has run
    const ncclResult_t r = ncclCommDestroy(ctx->comm);
    ctx->comm = nullptr;
    if (r != ncclSuccess) return nccl_fail(ctx, r, "ncclCommDestroy");
  }
  ctx->comm_rank = 0;
  ctx->comm_world = 1;
  return 0;
}

int bls_comm_abort(bls_ctx* ctx) {
  API_ENTER(ctx);
  return comm_abort_locked(ctx);
}

// The verdict of job `job`'s combined check: its partial all-gathered with every rank's and the product
// final-exponentiated, both enqueued by its submit (enqueue_comm_check), so this only waits for the 4-byte
// verdict: 1 / 0.  The host never sees the partials.  Every rank submits the same jobs in the same order.
static int job_check_comm(bls_ctx* ctx) {
  Job& J = *ctx->j;
  if (J.comm_pending) {  // enqueued by job_submit: only the verdict is left to read
    HIPCK(hipEventSynchronize(J.ev[EV_CV]));
    J.comm_pending = false;
    J.partial_pending = false;
    return J.h_own[1] ? 1 : 0;
  }
  if (!J.partial_pending || !J.buf[S_BYTES].p) {
    ctx->err = "no submitted FAV batch on this job";
    return BLS_E_ARG;
  }
  // a job submitted before the communicator existed: the exchange now (every rank must do the same)
  CK(enqueue_comm_check(ctx));
  return job_check_comm(ctx);
}

int bls_fav_job_check_comm(bls_ctx* ctx, int job) {
  JOB_ENTER(ctx, job);
  if (!ctx->comm) {
    ctx->err = ctx->comm_abort_cause.empty()
                   ? "bls_comm_init was not called"
                   : "the RCCL communicator was aborted after an earlier failure: " + ctx->comm_abort_cause;
    return BLS_E_ARG;
  }
  const int r = job_check_comm(ctx);
  if (r < 0) comm_fail_abort(ctx);
  return r;
}

}  // extern "C"
