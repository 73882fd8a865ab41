/* lgdistill.h — C ABI of the training side of teacher-student distillation: Distillation.update of the vendored rsl_rl
 * (algorithms/distillation.py:107-153, batches as storage/rollout_storage.py:170-182) for the feed-forward StudentTeacher, on the kernels of
 * lgtrain.h.  The trainer sits on ONE network that already exists, the student of a policy; the behaviour loss, the backward pass, the weight
 * gradients, the optional grad-norm clip and Adam run on the device and rewrite the tiled images the acts and collectors of lgpolicy.h read.
 * Same library and same conventions as lgtrain.h: device pointers unless marked HOST, asynchronous on the caller's hipStream_t unless a call copies
 * to the HOST, 0 / negative status, and ONE error channel: every refusal leaves "<entry point>: <reason>" in the thread's message (read with the
 * last-error call of lgpolicy.h) and launches nothing.
 *
 * An update walks the sequence of E * T steps (epoch 0 steps 0 .. T-1, epoch 1 steps 0 .. T-1, ...).  Step k has the loss
 * l_k = loss_fn(student(obs[t_k]), target[t_k]), an fp32 mean over N * A elements.  Every G = gradient_length consecutive steps form a group, which
 * may straddle an epoch boundary: one optimiser step on the gradient of the SUM of the group's losses, i.e. one batch of G * N rows.  The trailing
 * (E * T) mod G steps train nothing; they are run forward with the final weights and count in the reported mean.
 *
 * The recurrent student (StudentTeacherRecurrent: truncated BPTT through its memory) has a trainer of its own, lgdistill_recurrent.h.  Not built,
 * refused by the Python layer: multi-GPU reduction.
 * Equal inputs give equal bits: no atomics anywhere; every sum has a fixed order (per step: block order; across steps: step order). */
#ifndef LGDISTILL_H
#define LGDISTILL_H
#include <stdint.h>
#include "lgpolicy.h"
#ifdef __cplusplus
extern "C" {
#endif

enum lg_distill_loss { LG_LOSS_MSE = 0, LG_LOSS_HUBER = 1 };          /* huber: delta = 1, torch's default */

typedef struct lg_distill_train lg_distill_train;

typedef struct lg_distill_train_hyper {
  int32_t loss_type;                 /* lg_distill_loss */
  float max_grad_norm;               /* <= 0: no clip (the reference's max_grad_norm of None or 0) */
} lg_distill_train_hyper;

/* What an update reports (device memory, float64): the mean of the E * T step losses (each an fp32 mean, summed as float64 in step order), the
 * number of optimiser steps the update took, and the global gradient norm of the last one (before the clip; unchanged if none was taken). */
typedef struct lg_distill_train_stats {
  double behavior;
  double optimizer_steps;
  double grad_norm;
} lg_distill_train_stats;

/* A trainer over the student network.  weights[l] (out, in) row-major and biases[l] (out): HOST, torch's layout; they become the fp32 masters Adam
 * updates, and the create call rewrites the student's tiled images from them.  Moments and step count start at zero.  max_rows: the largest
 * G * N a group may have (workspaces are sized for it).  The student must outlive the trainer.  Refused: NULL handle or pointers, max_rows < 1, a
 * learning rate that is not > 0, a network whose output activation is set. */
lg_distill_train* lg_distill_train_create(lg_mlp* student, const float* const* weights, const float* const* biases, double learning_rate, int64_t max_rows);
void lg_distill_train_destroy(lg_distill_train* trainer);

/* One optimiser step on num_steps consecutive steps.  observations (T, N, S), targets (T, N, A): time-major, contiguous.  Step s of the group reads
 * time index (first_step + s) mod T.  Refused: NULL handle or pointer, T, N or num_steps < 1, first_step < 0, num_steps * N > max_rows, an unknown
 * loss type. */
int lg_distill_train_group(lg_distill_train* trainer, const float* observations, const float* targets, int64_t T, int64_t N, int64_t first_step,
                           int64_t num_steps, const lg_distill_train_hyper* hyper, void* stream);

/* Distillation.update: floor(E * T / G) groups, then the remainder forward-only.  Nothing is synchronised: the whole update is enqueued; stats
 * (device, may be NULL) is written by the last kernel.  Refused as the group call, and for num_learning_epochs or gradient_length < 1 or
 * gradient_length * N > max_rows. */
int lg_distill_train_update(lg_distill_train* trainer, const float* observations, const float* targets, int64_t T, int64_t N,
                            int32_t num_learning_epochs, int32_t gradient_length, const lg_distill_train_hyper* hyper, lg_distill_train_stats* stats,
                            void* stream);

/* Number of floats of the flat parameter vector: the student's W0, b0, W1, b1, ... in torch's layout. */
int64_t lg_distill_train_parameter_count(lg_distill_train* trainer);

/* The last group's gradients BEFORE the clip (HOST, flat as above), its global norm, and its per-step losses (HOST, capacity floats; the call
 * returns LG_ERR_INVALID if the group had more steps).  Any of the three may be NULL.  Waits for `stream`. */
int lg_distill_train_gradients(lg_distill_train* trainer, float* gradients_host, float* global_norm_host, float* step_losses_host, int64_t capacity,
                               void* stream);

/* The student's outputs (rows, A) of the last group's (or remainder's) forward pass, in step-major order (HOST).  Waits for `stream`. */
int lg_distill_train_forward_outputs(lg_distill_train* trainer, float* actions_host, void* stream);

/* The E * T step losses of the last update (HOST, count floats; count must not exceed E * T).  Waits for `stream`. */
int lg_distill_train_step_losses(lg_distill_train* trainer, float* losses_host, int64_t count, void* stream);

/* Checkpoints, as the calls of lgtrain.h: all HOST, flat as above; any pointer of get_state may be NULL.  set_state also rewrites the tiled images. */
int lg_distill_train_get_parameters(lg_distill_train* trainer, float* parameters_host, void* stream);
int lg_distill_train_get_state(lg_distill_train* trainer, float* parameters_host, float* exp_avg_host, float* exp_avg_sq_host, int64_t* step_host,
                               double* learning_rate_host, void* stream);
int lg_distill_train_set_state(lg_distill_train* trainer, const float* parameters_host, const float* exp_avg_host, const float* exp_avg_sq_host,
                               int64_t step, double learning_rate, void* stream);
int lg_distill_train_set_learning_rate(lg_distill_train* trainer, double learning_rate, void* stream);

#ifdef __cplusplus
}
#endif
#endif
