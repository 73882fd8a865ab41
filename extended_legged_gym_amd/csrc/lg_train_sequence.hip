// lg_train_sequence.hip — the supervised sequence update of the three sequence trainers (lg_train_sequence_internal.h): feed-forward and recurrent
// distillation, and the terrain estimator.
//
//   seq_rows_kernel         the group's row index: row j of the batch is row j % N of time step (t0 + j / N) % T, so a group that wraps the epoch
//                           boundary is still one gathered batch.
//   seq_loss_kernel         one lane per (row, column) of a step (blockIdx.y: the step, so no block straddles two steps): d = out - target, the element
//                           loss (mse | huber, delta 1 | l1), the seed gradient into the last layer's delta buffer, and the block's sum by a fixed tree.
//   seq_loss_finish_kernel  per step the block sums in block order -> the fp32 mean; then the means in step order into a float64 sum, the step and
//                           optimiser-step counters, the group's and the update's loss vectors (each where its pointer is not NULL).
//   seq_stats_kernel        clears the update's sums / writes the stats.
//   seq_mask_rows_kernel    Memory.reset(dones): zero h (and c) in every layer for the rows whose episode ended.
// No host synchronisation and no atomics: equal inputs give equal bits.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "lg_device.h"
#include "lg_policy_internal.h"
#include "lg_train_sequence_internal.h"
#include "../../include/lgdistill.h"
#include "../../include/lgestimator_train.h"

#define SEQ_LOSS_LANES 256

static_assert(SEQ_LOSS_MSE == LG_LOSS_MSE && SEQ_LOSS_HUBER == LG_LOSS_HUBER, "lg_distill_loss");
static_assert(SEQ_LOSS_MSE == LG_EST_LOSS_MSE && SEQ_LOSS_HUBER == LG_EST_LOSS_HUBER && SEQ_LOSS_L1 == LG_EST_LOSS_L1, "lg_estimator_loss");

__global__ __launch_bounds__(256) void seq_rows_kernel(int64_t* __restrict__ rows, int64_t count, int64_t N, int64_t T, int64_t t0) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j < count) rows[j] = ((t0 + j / N) % T) * N + j % N;
}

// out (steps, NW): the outputs in batch order, NW = N * out_w; target (T, NW).  delta (may be NULL: forward only) gets dl / dout of the SUM of the
// steps' means.  part[step][block]: the block's sum of element losses.
__global__ __launch_bounds__(SEQ_LOSS_LANES) void seq_loss_kernel(const float* __restrict__ out, const float* __restrict__ target, int64_t NW, int64_t T, int64_t t0,
                                                                  int loss_type, float* __restrict__ delta, float* __restrict__ part) {
  __shared__ float red[SEQ_LOSS_LANES];
  const int64_t s = blockIdx.y, e = (int64_t)blockIdx.x * SEQ_LOSS_LANES + threadIdx.x;
  float l = 0.f;
  if (e < NW) {
    const int64_t t = (t0 + s) % T;
    const float d = out[s * NW + e] - target[t * NW + e];
    const float inv = 1.f / (float)NW, ad = fabsf(d);
    float g;
    if (loss_type == SEQ_LOSS_HUBER) {                       // F.huber_loss, delta = 1
      l = ad < 1.f ? 0.5f * d * d : ad - 0.5f;
      g = ad < 1.f ? d : (d > 0.f ? 1.f : -1.f);
    } else if (loss_type == SEQ_LOSS_L1) {                   // F.l1_loss: sign(0) = 0
      l = ad;
      g = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
    } else {
      l = d * d;
      g = 2.f * d;
    }
    if (delta) delta[s * NW + e] = g * inv;
  }
  const float sum = block_sum_256(l, red);
  if (threadIdx.x == 0) part[(size_t)s * gridDim.x + blockIdx.x] = sum;
}

// One block.  train != 0: the steps were a group (counts an optimiser step).  group_loss, seq_loss (either may be NULL): the last group's loss vector;
// the update's, at the offset of the group's first step.
__global__ __launch_bounds__(256) void seq_loss_finish_kernel(const float* __restrict__ part, int nblocks, int64_t nsteps, int64_t NW, float* __restrict__ step_tmp,
                                                              float* __restrict__ group_loss, float* __restrict__ seq_loss, SeqScalars* __restrict__ ss, int train) {
  for (int64_t s = threadIdx.x; s < nsteps; s += 256) {
    float sum = 0.f;
    for (int b = 0; b < nblocks; ++b) sum += part[(size_t)s * nblocks + b];
    step_tmp[s] = sum / (float)NW;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double acc = ss->acc;
  for (int64_t s = 0; s < nsteps; ++s) {
    const float v = step_tmp[s];
    acc += (double)v;
    if (group_loss) group_loss[s] = v;
    if (seq_loss) seq_loss[s] = v;
  }
  ss->acc = acc;
  ss->steps += nsteps;
  if (train) ss->optimizer_steps += 1;
}

// mode 0: clear the update's sums; 1: write the stats {mean, optimiser steps, gradient norm} and, with extra, a fourth double from it
__global__ void seq_stats_kernel(SeqScalars* __restrict__ ss, const TrainScalars* __restrict__ sc, const float* __restrict__ extra, double* __restrict__ stats, int mode) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (mode == 0) { ss->acc = 0.0; ss->steps = 0; ss->optimizer_steps = 0; return; }
  stats[0] = ss->acc / (double)ss->steps;
  stats[1] = (double)ss->optimizer_steps;
  stats[2] = (double)sc->norm;
  if (extra) stats[3] = (double)*extra;
}

__global__ __launch_bounds__(256) void seq_mask_rows_kernel(float* __restrict__ h, float* __restrict__ c, const float* __restrict__ dones, int64_t N, int H,
                                                            int64_t layer_stride, int layers) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= N * H) return;
  if (dones[idx / H] != 0.f)
    for (int l = 0; l < layers; ++l) { h[l * layer_stride + idx] = 0.f; if (c) c[l * layer_stride + idx] = 0.f; }
}

// ------------------------------------------------------------------------------------------------------------------------ host side
bool seq_alloc(SeqCore* c, int64_t max_rows, int out_w, bool want_rows) {
  bool ok = true;
  auto alloc = [&](size_t bytes) -> void* { void* d = ok ? train_alloc(c, bytes, true) : nullptr; if (!d) ok = false; return d; };
  const size_t R = (size_t)max_rows;
  c->out_w = out_w;
  // a step has ceil(N out_w / 256) blocks and a batch at most max_rows steps: at most max_rows out_w / 256 + max_rows blocks in all
  c->loss_part = (float*)alloc((R * out_w / SEQ_LOSS_LANES + R + 1) * sizeof(float));
  if (want_rows) c->rows = (int64_t*)alloc(R * sizeof(int64_t));
  c->step_tmp = (float*)alloc(R * sizeof(float));
  c->group_loss = (float*)alloc(R * sizeof(float));
  c->seq_cap = 1024;
  c->seq_loss = (float*)alloc((size_t)c->seq_cap * sizeof(float));
  c->ss = (SeqScalars*)alloc(sizeof(SeqScalars));
  return ok;
}

void seq_launch_rows(int64_t* rows, int64_t n, int64_t N, int64_t T, int64_t t0, hipStream_t st) {
  hipLaunchKernelGGL(seq_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, rows, n, N, T, t0);
}

void seq_launch_loss(SeqCore* c, const float* out, const float* tgt, int64_t N, int64_t T, int64_t t0, int64_t nsteps, int loss_type, float* delta, float* group_loss,
                     float* seq_loss, int train, hipStream_t st) {
  const int64_t NW = N * c->out_w;
  const int nblocks = (int)((NW + SEQ_LOSS_LANES - 1) / SEQ_LOSS_LANES);
  hipLaunchKernelGGL(seq_loss_kernel, dim3(nblocks, (unsigned)nsteps), dim3(SEQ_LOSS_LANES), 0, st, out, tgt, NW, T, t0, loss_type, delta, c->loss_part);
  hipLaunchKernelGGL(seq_loss_finish_kernel, dim3(1), dim3(256), 0, st, (const float*)c->loss_part, nblocks, nsteps, NW, c->step_tmp, group_loss, seq_loss, c->ss, train);
}

void seq_launch_mask_rows(float* h, float* c, const float* dones, int64_t N, int H, int64_t layer_stride, int layers, hipStream_t st) {
  hipLaunchKernelGGL(seq_mask_rows_kernel, dim3((unsigned)((N * H + 255) / 256)), dim3(256), 0, st, h, c, dones, N, H, layer_stride, layers);
}

int seq_check_group(const SeqCore* c, int64_t N, int64_t first_step, int64_t num_steps) {
  if (num_steps < 1 || first_step < 0) return lg_policy_fail(LG_ERR_INVALID, "num_steps < 1 or first_step < 0");
  if (num_steps > SEQ_MAX_STEPS) return lg_policy_fail(LG_ERR_INVALID, "num_steps > 65535");
  if (N > c->max_rows || num_steps > c->max_rows / N) return lg_policy_fail(LG_ERR_INVALID, "num_steps * N > max_rows of the trainer");
  return LG_OK;
}

int seq_update(SeqCore* c, int64_t T, int64_t N, int32_t E, int32_t G, const SeqSteps& run_steps, TrainMem* mem, void* stats, const float* extra_norm, void* stream) {
  if (E < 1 || G < 1) return lg_policy_fail(LG_ERR_INVALID, "num_learning_epochs < 1 or gradient_length < 1");
  if (G > SEQ_MAX_STEPS) return lg_policy_fail(LG_ERR_INVALID, "gradient_length > 65535");
  if (N > c->max_rows || G > c->max_rows / N) return lg_policy_fail(LG_ERR_INVALID, "gradient_length * N > max_rows of the trainer");
  DeviceScope ds_(c->device);
  hipStream_t st = (hipStream_t)stream;
  const int64_t total = (int64_t)E * T;
  if (total > c->seq_cap) {                                  // (the old vector stays with the trainer: kernels in flight may still write it)
    float* grown = (float*)train_alloc(c, (size_t)total * sizeof(float), true);
    if (!grown) return LG_ERR_HIP;
    c->seq_loss = grown; c->seq_cap = total;
  }
  c->last_update_steps = total;
  hipLaunchKernelGGL(seq_stats_kernel, dim3(1), dim3(1), 0, st, c->ss, (const TrainScalars*)c->sc, extra_norm, (double*)stats, 0);
  int64_t k = 0;
  int rc = LG_OK;
  for (; total - k >= G; k += G)                             // whole groups: an optimiser step each
    if ((rc = run_steps(k, G, true, c->seq_loss + k, st)) != LG_OK) return rc;
  if (k < total && (rc = run_steps(k, total - k, false, c->seq_loss + k, st)) != LG_OK) return rc;          // the remainder: forward and losses only
  if (mem && (rc = mem_keep_carry(mem, st)) != LG_OK) return rc;
  if (stats) hipLaunchKernelGGL(seq_stats_kernel, dim3(1), dim3(1), 0, st, c->ss, (const TrainScalars*)c->sc, extra_norm, (double*)stats, 1);
  POLICY_TRY(hipGetLastError());
  return LG_OK;
}

int seq_forward_outputs(SeqCore* c, float* out, void* stream) {
  if (!c || !out) return lg_policy_fail(LG_ERR_INVALID, "null trainer or buffer");
  if (c->last_rows <= 0) return lg_policy_fail(LG_ERR_INVALID, "no group has run yet");
  DeviceScope ds_(c->device);
  POLICY_TRY(hipStreamSynchronize((hipStream_t)stream));
  const TrainNet& S = c->net[0];
  POLICY_TRY(hipMemcpy(out, S.a[S.L], (size_t)c->last_rows * c->out_w * sizeof(float), hipMemcpyDeviceToHost));
  return LG_OK;
}
