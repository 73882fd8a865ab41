// lg_distill_train.hip — Distillation.update (include/lgdistill.h) for the feed-forward StudentTeacher: a trainer over ONE lg_mlp, the student.
// A group of G steps is one batch of G * N rows through the kernels of lg_train.hip (forward with saved activations, backward data pass, weight
// gradients by slabs, reduce, norm, Adam with the rewrite of the tilings), launched with one network, between the row index and the behaviour loss of
// lg_train_sequence.hip (lg_train_sequence_internal.h), whose seq_update is the update's loop.  No kernel lives here.
// An optimiser step is nine launches, a forward-only remainder four; no host synchronisation and no atomics: equal inputs give equal bits.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string>
#include <vector>

#include "lg_device.h"
#include "lg_policy_internal.h"
#include "lg_train_internal.h"
#include "lg_train_sequence_internal.h"
#include "../../include/lgdistill.h"

struct lg_distill_train : SeqCore {
  lg_mlp* student = nullptr;
};

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
  const int64_t n = nsteps * N, t0 = first % T;
  const TrainNet& S = p->net[0];
  p->last_rows = n;
  if (train) p->last_steps = nsteps;                         // a forward-only remainder leaves the last group's count and its group_loss alone
  seq_launch_rows(p->rows, n, N, T, t0, st);
  train_launch_forward(p, obs, obs, p->rows, n, st);
  seq_launch_loss(p, S.a[S.L], tgt, N, T, t0, nsteps, h->loss_type, train ? S.d[S.L - 1] : (float*)nullptr, train ? p->group_loss : (float*)nullptr, seq_loss,
                  train ? 1 : 0, st);
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
  p->student = student; p->device = student->device; p->max_rows = max_rows;
  int64_t off = 0;
  const bool ok = train_core_add_net(p, student, &off) && seq_alloc(p, max_rows, student->h.dims[student->h.L], true);
  const float* const* ws[1] = {weights};
  const float* const* bs[1] = {biases};
  if (!ok || train_core_finish(p, off, ws, bs, nullptr, learning_rate) != LG_OK) { lg_distill_train_destroy(p); return nullptr; }
  return p;
}

int lg_distill_train_group(lg_distill_train* p, const float* obs, const float* tgt, int64_t T, int64_t N, int64_t first_step, int64_t num_steps,
                           const lg_distill_train_hyper* hyper, void* stream) {
  POLICY_ENTRY;
  int rc = distill_check_call(p, obs, tgt, T, N, hyper);
  if (rc != LG_OK) return rc;
  if ((rc = seq_check_group(p, N, first_step, num_steps)) != LG_OK) return rc;
  DeviceScope ds_(p->device);
  return distill_steps(p, obs, tgt, T, N, first_step, num_steps, hyper, true, nullptr, (hipStream_t)stream);
}

int lg_distill_train_update(lg_distill_train* p, const float* obs, const float* tgt, int64_t T, int64_t N, int32_t E, int32_t G, const lg_distill_train_hyper* hyper,
                            lg_distill_train_stats* stats, void* stream) {
  POLICY_ENTRY;
  const int rc = distill_check_call(p, obs, tgt, T, N, hyper);
  if (rc != LG_OK) return rc;
  return seq_update(p, T, N, E, G, [&](int64_t first, int64_t nsteps, bool train, float* seq_loss, hipStream_t st) {
    return distill_steps(p, obs, tgt, T, N, first, nsteps, hyper, train, seq_loss, st); }, nullptr, stats, nullptr, stream);
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
  return seq_forward_outputs(p, actions, stream);
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
