// lg_distill_train.hip — Distillation.update (include/lgdistill.h) for the feed-forward StudentTeacher: a trainer over ONE lg_mlp, the student.
// A group of G steps is one batch of G * N rows through the kernels of lg_train.hip (forward with saved activations, backward data pass, weight
// gradients by slabs, reduce, norm, Adam with the rewrite of the tilings), launched with one network; what is new here:
//
//   distill_rows_kernel         the group's row index: row j of the batch is row j % N of time step (t0 + j / N) % T, so a group that wraps the
//                               epoch boundary is still one gathered batch.
//   distill_loss_kernel         one lane per (row, action) of a step (blockIdx.y: the step, so no block straddles two steps): d = student - target,
//                               the element loss (mse | huber, delta 1), the seed gradient into the last layer's delta buffer, and the block's sum
//                               by a fixed tree.
//   distill_loss_finish_kernel  per step the block sums in block order -> the fp32 mean; then the means in step order into a float64 sum, the
//                               step and optimiser-step counters, the group's and the update's loss vectors.
//   distill_stats_kernel        clears the update's sums / writes the stats.
// An optimiser step is nine launches, a forward-only remainder four; no host synchronisation and no atomics: equal inputs give equal bits.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string>
#include <vector>

#include "lg_device.h"
#include "lg_policy_internal.h"
#include "lg_train_internal.h"
#include "lg_distill_train_internal.h"
#include "../../include/lgdistill.h"

#define DISTILL_LOSS_LANES 256
#define DISTILL_MAX_STEPS 65535     // steps of one batch: blockIdx.y of the loss kernel

// DistillScalars: lg_distill_train_internal.h

struct lg_distill_train : TrainCore {
  lg_mlp* student = nullptr;
  int A = 0;
  int64_t seq_cap = 0;               // last_steps, last_update_steps, group_loss (max_rows) and seq_loss (seq_cap) are the core's
  int64_t* rows = nullptr;           // (max_rows) the group's row index
  float* loss_part = nullptr;        // [step][block]
  float* step_tmp = nullptr;         // (max_rows) the means of the steps in flight
  DistillScalars* ds = nullptr;
};

__global__ __launch_bounds__(256) void distill_rows_kernel(int64_t* __restrict__ rows, int64_t count, int64_t N, int64_t T, int64_t t0) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j < count) rows[j] = ((t0 + j / N) % T) * N + j % N;
}

// out (steps, N * A): the student's outputs in batch order; target (T, N * A).  delta (may be NULL: forward only) gets dl / dout of the SUM of the
// steps' means.  part[step][block]: the block's sum of element losses.
__global__ __launch_bounds__(DISTILL_LOSS_LANES) void distill_loss_kernel(const float* __restrict__ out, const float* __restrict__ target, int64_t NA, int64_t T,
                                                                          int64_t t0, int loss_type, float* __restrict__ delta, float* __restrict__ part) {
  __shared__ float red[DISTILL_LOSS_LANES];
  const int64_t s = blockIdx.y, e = (int64_t)blockIdx.x * DISTILL_LOSS_LANES + threadIdx.x;
  float l = 0.f;
  if (e < NA) {
    const int64_t t = (t0 + s) % T;
    const float d = out[s * NA + e] - target[t * NA + e];
    const float inv = 1.f / (float)NA;
    float g;
    if (loss_type == LG_LOSS_HUBER) {                        // F.huber_loss, delta = 1
      const float ad = fabsf(d);
      l = ad < 1.f ? 0.5f * d * d : ad - 0.5f;
      g = ad < 1.f ? d : (d > 0.f ? 1.f : -1.f);
    } else {
      l = d * d;
      g = 2.f * d;
    }
    if (delta) delta[s * NA + e] = g * inv;
  }
  const float sum = block_sum_256(l, red);
  if (threadIdx.x == 0) part[(size_t)s * gridDim.x + blockIdx.x] = sum;
}

// One block.  train != 0: the steps were a group (counts an optimiser step, fills group_loss).  seq_loss (may be NULL): the update's loss vector, at
// the offset of the group's first step.
__global__ __launch_bounds__(256) void distill_loss_finish_kernel(const float* __restrict__ part, int nblocks, int64_t nsteps, int64_t NA, float* __restrict__ step_tmp,
                                                                  float* __restrict__ group_loss, float* __restrict__ seq_loss, DistillScalars* __restrict__ ds,
                                                                  int train) {
  for (int64_t s = threadIdx.x; s < nsteps; s += 256) {
    float sum = 0.f;
    for (int b = 0; b < nblocks; ++b) sum += part[(size_t)s * nblocks + b];
    step_tmp[s] = sum / (float)NA;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double acc = ds->acc;
  for (int64_t s = 0; s < nsteps; ++s) {
    const float v = step_tmp[s];
    acc += (double)v;
    if (train) group_loss[s] = v;
    if (seq_loss) seq_loss[s] = v;
  }
  ds->acc = acc;
  ds->steps += nsteps;
  if (train) ds->optimizer_steps += 1;
}

// mode 0: clear the update's sums; 1: write the stats
__global__ void distill_stats_kernel(DistillScalars* __restrict__ ds, const TrainScalars* __restrict__ sc, lg_distill_train_stats* __restrict__ stats, int mode) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (mode == 0) { ds->acc = 0.0; ds->steps = 0; ds->optimizer_steps = 0; return; }
  stats->behavior = ds->acc / (double)ds->steps;
  stats->optimizer_steps = (double)ds->optimizer_steps;
  stats->grad_norm = (double)sc->norm;
}

// ------------------------------------------------------------------------------------------------------------------------ host side
// ---- what the recurrent trainer shares (lg_distill_train_internal.h)
size_t distill_loss_floats(int64_t max_rows, int A) { return (size_t)max_rows * A / DISTILL_LOSS_LANES + (size_t)max_rows + 1; }

void distill_launch_rows(int64_t* rows, int64_t n, int64_t N, int64_t T, int64_t t0, hipStream_t st) {
  hipLaunchKernelGGL(distill_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, rows, n, N, T, t0);
}

void distill_launch_loss(const float* out, const float* tgt, int64_t N, int A, int64_t T, int64_t t0, int64_t nsteps, int loss_type, float* delta, float* loss_part,
                         float* step_tmp, float* group_loss, float* seq_loss, DistillScalars* ds, int train, hipStream_t st) {
  const int64_t NA = N * A;
  const int nblocks = (int)((NA + DISTILL_LOSS_LANES - 1) / DISTILL_LOSS_LANES);
  hipLaunchKernelGGL(distill_loss_kernel, dim3(nblocks, (unsigned)nsteps), dim3(DISTILL_LOSS_LANES), 0, st, out, tgt, NA, T, t0, loss_type, delta, loss_part);
  hipLaunchKernelGGL(distill_loss_finish_kernel, dim3(1), dim3(256), 0, st, (const float*)loss_part, nblocks, nsteps, NA, step_tmp, group_loss, seq_loss, ds, train);
}

static int distill_check_call(lg_distill_train* p, const float* obs, const float* tgt, int64_t T, int64_t N, const lg_distill_train_hyper* h) {
  if (!p) return lg_policy_fail(LG_ERR_INVALID, "null trainer");
  if (!obs || !tgt || !h) return lg_policy_fail(LG_ERR_INVALID, "null observations, targets or hyper-parameters");
  if (T < 1 || N < 1) return lg_policy_fail(LG_ERR_INVALID, "T < 1 or N < 1");
  if (h->loss_type != LG_LOSS_MSE && h->loss_type != LG_LOSS_HUBER) return lg_policy_fail(LG_ERR_INVALID, "unknown loss type (mse | huber)");
  return LG_OK;
}

// steps [first, first + nsteps) of the sequence as one batch; train: an optimiser step, else forward and loss only.  seq_loss: where the update keeps
// these steps' losses, or NULL.
static int distill_steps(lg_distill_train* p, const float* obs, const float* tgt, int64_t T, int64_t N, int64_t first, int64_t nsteps, const lg_distill_train_hyper* h,
                         bool train, float* seq_loss, hipStream_t st) {
  const int64_t n = nsteps * N, NA = N * p->A, t0 = first % T;
  const TrainNet& S = p->net[0];
  const int nblocks = (int)((NA + DISTILL_LOSS_LANES - 1) / DISTILL_LOSS_LANES);
  p->last_rows = n;
  if (train) p->last_steps = nsteps;
  hipLaunchKernelGGL(distill_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, p->rows, n, N, T, t0);
  train_launch_forward(p, obs, obs, p->rows, n, st);
  hipLaunchKernelGGL(distill_loss_kernel, dim3(nblocks, (unsigned)nsteps), dim3(DISTILL_LOSS_LANES), 0, st, (const float*)S.a[S.L], tgt, NA, T, t0, h->loss_type,
                     train ? S.d[S.L - 1] : (float*)nullptr, p->loss_part);
  hipLaunchKernelGGL(distill_loss_finish_kernel, dim3(1), dim3(256), 0, st, (const float*)p->loss_part, nblocks, nsteps, NA, p->step_tmp, p->group_loss, seq_loss, p->ds,
                     train ? 1 : 0);
  if (!train) { POLICY_TRY(hipGetLastError()); return LG_OK; }
  train_launch_backward(p, n, st);
  return train_launch_optimise(p, obs, obs, p->rows, n, h->max_grad_norm, h->max_grad_norm > 0.f ? 1 : 0, st);
}

extern "C" {

void lg_distill_train_destroy(lg_distill_train* p) {
  if (!p) return;
  DeviceScope ds_(p->device);
  (void)hipDeviceSynchronize();
  train_core_free(p);
  delete p;
}

lg_distill_train* lg_distill_train_create(lg_mlp* student, const float* const* weights, const float* const* biases, double learning_rate, int64_t max_rows) {
  POLICY_ENTRY;
  if (!student) { lg_policy_fail(LG_ERR_INVALID, "null network"); return nullptr; }
  if (!weights || !biases) { lg_policy_fail(LG_ERR_INVALID, "null parameter list"); return nullptr; }
  if (max_rows < 1) { lg_policy_fail(LG_ERR_INVALID, "max_rows < 1"); return nullptr; }
  if (!(learning_rate > 0.0)) { lg_policy_fail(LG_ERR_INVALID, "learning rate <= 0"); return nullptr; }
  if (student->h.act_out) { lg_policy_fail(LG_ERR_UNSUPPORTED, "a network with an output activation cannot be trained here"); return nullptr; }
  for (int l = 0; l < student->h.L; ++l)
    if (!weights[l] || !biases[l]) { lg_policy_fail(LG_ERR_INVALID, "null weight or bias"); return nullptr; }
  if (!lg_policy_device_ok(student->device)) return nullptr;
  DeviceScope ds_(student->device);
  if (!ds_.ok) { lg_policy_fail(LG_ERR_INVALID, "bad device"); return nullptr; }
  lg_distill_train* p = new lg_distill_train();
  p->student = student; p->device = student->device; p->A = student->h.dims[student->h.L]; p->max_rows = max_rows;
  int64_t off = 0;
  bool ok = train_core_add_net(p, student, &off);
  auto alloc = [&](size_t bytes) -> void* { void* d = ok ? train_alloc(p, bytes, true) : nullptr; if (!d) ok = false; return d; };
  // a step has ceil(N A / 256) blocks and a batch at most max_rows steps: at most max_rows A / 256 + max_rows blocks in all
  p->loss_part = (float*)alloc(((size_t)max_rows * p->A / DISTILL_LOSS_LANES + (size_t)max_rows + 1) * sizeof(float));
  p->rows = (int64_t*)alloc((size_t)max_rows * sizeof(int64_t));
  p->step_tmp = (float*)alloc((size_t)max_rows * sizeof(float));
  p->group_loss = (float*)alloc((size_t)max_rows * sizeof(float));
  p->seq_cap = 1024;
  p->seq_loss = (float*)alloc((size_t)p->seq_cap * sizeof(float));
  p->ds = (DistillScalars*)alloc(sizeof(DistillScalars));
  const float* const* ws[1] = {weights};
  const float* const* bs[1] = {biases};
  if (!ok || train_core_finish(p, off, ws, bs, nullptr, learning_rate) != LG_OK) { lg_distill_train_destroy(p); return nullptr; }
  return p;
}

int lg_distill_train_group(lg_distill_train* p, const float* obs, const float* tgt, int64_t T, int64_t N, int64_t first_step, int64_t num_steps,
                           const lg_distill_train_hyper* hyper, void* stream) {
  POLICY_ENTRY;
  const int rc = distill_check_call(p, obs, tgt, T, N, hyper);
  if (rc != LG_OK) return rc;
  if (num_steps < 1 || first_step < 0) return lg_policy_fail(LG_ERR_INVALID, "num_steps < 1 or first_step < 0");
  if (num_steps > DISTILL_MAX_STEPS) return lg_policy_fail(LG_ERR_INVALID, "num_steps > 65535");
  if (N > p->max_rows || num_steps > p->max_rows / N) return lg_policy_fail(LG_ERR_INVALID, "num_steps * N > max_rows of the trainer");
  DeviceScope ds_(p->device);
  return distill_steps(p, obs, tgt, T, N, first_step, num_steps, hyper, true, nullptr, (hipStream_t)stream);
}

int lg_distill_train_update(lg_distill_train* p, const float* obs, const float* tgt, int64_t T, int64_t N, int32_t E, int32_t G, const lg_distill_train_hyper* hyper,
                            lg_distill_train_stats* stats, void* stream) {
  POLICY_ENTRY;
  const int rc = distill_check_call(p, obs, tgt, T, N, hyper);
  if (rc != LG_OK) return rc;
  if (E < 1 || G < 1) return lg_policy_fail(LG_ERR_INVALID, "num_learning_epochs < 1 or gradient_length < 1");
  if (G > DISTILL_MAX_STEPS) return lg_policy_fail(LG_ERR_INVALID, "gradient_length > 65535");
  if (N > p->max_rows || G > p->max_rows / N) return lg_policy_fail(LG_ERR_INVALID, "gradient_length * N > max_rows of the trainer");
  DeviceScope ds_(p->device);
  hipStream_t st = (hipStream_t)stream;
  const int64_t total = (int64_t)E * T;
  if (total > p->seq_cap) {                                  // (the old vector stays with the trainer: kernels in flight may still write it)
    float* grown = (float*)train_alloc(p, (size_t)total * sizeof(float), true);
    if (!grown) return LG_ERR_HIP;
    p->seq_loss = grown; p->seq_cap = total;
  }
  p->last_update_steps = total;
  hipLaunchKernelGGL(distill_stats_kernel, dim3(1), dim3(1), 0, st, p->ds, (const TrainScalars*)p->sc, stats, 0);
  int64_t k = 0;
  for (; total - k >= G; k += G) {
    const int r2 = distill_steps(p, obs, tgt, T, N, k, G, hyper, true, p->seq_loss + k, st);
    if (r2 != LG_OK) return r2;
  }
  if (k < total) {
    const int r2 = distill_steps(p, obs, tgt, T, N, k, total - k, hyper, false, p->seq_loss + k, st);
    if (r2 != LG_OK) return r2;
  }
  if (stats) hipLaunchKernelGGL(distill_stats_kernel, dim3(1), dim3(1), 0, st, p->ds, (const TrainScalars*)p->sc, stats, 1);
  POLICY_TRY(hipGetLastError());
  return LG_OK;
}

int64_t lg_distill_train_parameter_count(lg_distill_train* p) {
  POLICY_ENTRY;
  return train_api_parameter_count(p);
}

int lg_distill_train_gradients(lg_distill_train* p, float* g, float* norm, float* losses, int64_t capacity, void* stream) {
  POLICY_ENTRY;
  return train_api_group_gradients(p, g, norm, losses, capacity, stream);
}

int lg_distill_train_forward_outputs(lg_distill_train* p, float* actions, void* stream) {
  POLICY_ENTRY;
  if (!p || !actions) return lg_policy_fail(LG_ERR_INVALID, "null trainer or buffer");
  if (p->last_rows <= 0) return lg_policy_fail(LG_ERR_INVALID, "no group has run yet");
  DeviceScope ds_(p->device);
  POLICY_TRY(hipStreamSynchronize((hipStream_t)stream));
  const TrainNet& S = p->net[0];
  POLICY_TRY(hipMemcpy(actions, S.a[S.L], (size_t)p->last_rows * p->A * sizeof(float), hipMemcpyDeviceToHost));
  return LG_OK;
}

int lg_distill_train_step_losses(lg_distill_train* p, float* losses, int64_t count, void* stream) {
  POLICY_ENTRY;
  return train_api_step_losses(p, losses, count, stream);
}

int lg_distill_train_get_state(lg_distill_train* p, float* params, float* exp_avg, float* exp_avg_sq, int64_t* step, double* lr, void* stream) {
  POLICY_ENTRY;
  return train_api_get_state(p, params, exp_avg, exp_avg_sq, step, lr, stream);
}

int lg_distill_train_get_parameters(lg_distill_train* p, float* params, void* stream) {
  POLICY_ENTRY;
  return train_api_get_parameters(p, params, stream);
}

int lg_distill_train_set_state(lg_distill_train* p, const float* params, const float* exp_avg, const float* exp_avg_sq, int64_t step, double lr, void* stream) {
  POLICY_ENTRY;
  return train_api_set_state(p, params, exp_avg, exp_avg_sq, step, lr, stream);
}

int lg_distill_train_set_learning_rate(lg_distill_train* p, double lr, void* stream) {
  POLICY_ENTRY;
  return train_api_set_learning_rate(p, lr, stream);
}

}  // extern "C"
