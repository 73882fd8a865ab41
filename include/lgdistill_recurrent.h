/* lgdistill_recurrent.h — C ABI of Distillation.update of the vendored rsl_rl (algorithms/distillation.py:107-153) for the recurrent student,
 * StudentTeacherRecurrent (modules/student_teacher_recurrent.py:71-100, networks/memory.py:35-65): truncated BPTT through the student's memory.  The
 * trainer sits on the TWO handles of a student that already exists (lgpolicy.h): its memory (lg_rnn) and its MLP (lg_mlp).  Forward with saved gates,
 * the behaviour loss, the backward pass through the MLP and through the memory in time, the weight gradients, the optional grad-norm clip and Adam
 * run on the device and rewrite the images lg_rnn_step, lg_mlp_forward, lg_distill_act_recurrent and lg_collect_distillation_recurrent read.  Same
 * library and conventions as lgdistill.h: device pointers unless marked HOST, asynchronous on the caller's hipStream_t unless a call copies to the
 * HOST, 0 / negative status, and ONE error channel: every refusal leaves "<entry point>: <reason>" in the thread's message (lg_mlp_last_error of
 * lgpolicy.h) and launches nothing.
 *
 * An update walks E * T steps, epoch-major.  Step k reads time index t_k = k mod T of observations (T, N, S), targets (T, N, A) and dones (T, N);
 * its loss l_k = loss_fn(student(memory(obs[t_k])), target[t_k]) is an fp32 mean over N * A elements.  Every G = gradient_length consecutive steps
 * form a group, which may straddle an epoch boundary: one optimiser step on the gradient of the SUM of the group's losses.  The trailing
 * (E * T) mod G steps run forward only with the final weights; they count in the reported mean and advance the memory.
 *
 * The memory.  Gradients flow through the memory inside a group only (truncated BPTT); a group's first step enters with the running state as a
 * constant.  Dones are always applied: after step k the rows with dones[t_k] != 0 are zeroed in every layer, and no gradient crosses into the step
 * before.  A step with t_k = 0 (the first of every epoch) enters with the CARRY as a constant: the state the last update ended with, zeros before
 * the first -- every epoch re-seeds from the carry the update started with, not from the previous epoch's end (distillation.py:114).  After an
 * update the carry is the running state after the last step's dones were applied.  The trainer owns the carry (L, N, H) (+ c for an LSTM) and the
 * running state; the live inference state of the memory's other callers is not touched.
 *
 * The clip covers the MLP only (distillation.py:136 clips policy.student.parameters()): its norm is taken over student.* alone and its scale is
 * applied to student.* alone; the gradients of memory_s.* enter Adam unscaled.  Both norms are reported.
 *
 * Parameters: one flat fp32 vector, each tensor in torch's layout: student.{i} (weight, bias) per layer, then
 * memory_s.rnn.{weight_ih, weight_hh, bias_ih, bias_hh}_l{l} per layer -- the order StudentTeacherRecurrent.state_dict() lists the trained tensors.
 * Adam (torch's defaults) runs over all of it; the teacher, its memory and std are not the trainer's.
 *
 * Workspace.  The saved gates of a group are KEPT: per row of a group (a row = one env of one step) and memory layer 4 H of gates, h_in, h', dL/dh'
 * (+ c_in, c' for an LSTM) and G H (LSTM) or 2 G H (GRU) gate derivatives, plus the MLP's activations and deltas.
 *
 * Equal inputs give equal bits: no atomics anywhere; every sum has a fixed order. */
#ifndef LGDISTILL_RECURRENT_H
#define LGDISTILL_RECURRENT_H
#include <stdint.h>
#include "lgdistill.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct lg_distill_rtrain lg_distill_rtrain;

/* HOST pointers to the trained tensors in torch's layout.  student_*[layers of the student handle]; memory_*[num_layers of the memory handle]. */
typedef struct lg_distill_rtrain_params {
  const float* const* student_weights; const float* const* student_biases;
  const float* const* memory_w_ih; const float* const* memory_w_hh; const float* const* memory_b_ih; const float* const* memory_b_hh;
} lg_distill_rtrain_params;

/* What an update reports (device memory, float64): the mean of the E * T step losses (each an fp32 mean, summed as float64 in step order), the number
 * of optimiser steps, and of the last one the gradient norm over student.* (before the clip: the norm the clip uses) and the norm over memory_s.*
 * (both unchanged if no step was taken). */
typedef struct lg_distill_rtrain_stats {
  double behavior;
  double optimizer_steps;
  double grad_norm;
  double memory_grad_norm;
} lg_distill_rtrain_stats;

/* A trainer over the student's memory and MLP, which must outlive it.  The HOST parameters become the fp32 masters Adam updates, and the create call
 * rewrites every device image from them.  Moments, step count and carry start at zero.  max_rows: the largest G * N a group may have.  Refused: a
 * NULL handle or pointer, max_rows < 1, a learning rate that is not > 0, an MLP whose output activation is set or whose input width is not the
 * memory's hidden width, handles on different devices. */
lg_distill_rtrain* lg_distill_rtrain_create(lg_rnn* memory, lg_mlp* student, const lg_distill_rtrain_params* params, double learning_rate, int64_t max_rows);
void lg_distill_rtrain_destroy(lg_distill_rtrain* trainer);

/* num_steps consecutive steps from step first_step of the sequence (step s reads time index (first_step + s) mod T); train != 0: one optimiser step
 * on the sum of their losses, else forward and losses only (the remainder of an update).  observations (T, N, S), targets (T, N, A), dones (T, N):
 * time-major, contiguous.  A step with time index 0 enters with the carry, every other first step with the running state; the running state (dones
 * of the last step applied) is left after the last step, the carry is not written.  hyper: lg_distill_train_hyper of lgdistill.h.  Refused: NULL
 * handle or pointer, T, N or num_steps < 1, first_step < 0, num_steps * N > max_rows, an unknown loss type, an N that is not the carry's
 * (reset_carry first). */
int lg_distill_rtrain_group(lg_distill_rtrain* trainer, const float* observations, const float* targets, const float* dones, int64_t T, int64_t N,
                            int64_t first_step, int64_t num_steps, int32_t train, const lg_distill_train_hyper* hyper, void* stream);

/* Distillation.update: floor(E * T / G) groups, the remainder forward-only, then carry := the running state.  Nothing is synchronised; stats
 * (device, may be NULL) is written by the last kernel.  Refused as the group call, and for num_learning_epochs or gradient_length < 1 or
 * gradient_length * N > max_rows. */
int lg_distill_rtrain_update(lg_distill_rtrain* trainer, const float* observations, const float* targets, const float* dones, int64_t T, int64_t N,
                             int32_t num_learning_epochs, int32_t gradient_length, const lg_distill_train_hyper* hyper, lg_distill_rtrain_stats* stats,
                             void* stream);

/* Number of floats of the flat parameter vector, and of its leading student.* part; bytes of device memory the trainer holds. */
int64_t lg_distill_rtrain_parameter_count(lg_distill_rtrain* trainer);
int64_t lg_distill_rtrain_student_parameter_count(lg_distill_rtrain* trainer);
int64_t lg_distill_rtrain_workspace_bytes(lg_distill_rtrain* trainer);

/* The last group's gradients BEFORE the clip (HOST, flat as above), its two norms (norms_host[0]: student.*, [1]: memory_s.*), and its per-step
 * losses (HOST, capacity floats; LG_ERR_INVALID if the group had more steps).  Any of the three may be NULL.  Waits for `stream`. */
int lg_distill_rtrain_gradients(lg_distill_rtrain* trainer, float* gradients_host, float* norms_host, float* step_losses_host, int64_t capacity,
                                void* stream);
/* The student's outputs (rows, A) of the last group call's forward pass, step-major (HOST).  Waits for `stream`. */
int lg_distill_rtrain_forward_outputs(lg_distill_rtrain* trainer, float* actions_host, void* stream);
/* The E * T step losses of the last update (HOST, count floats; count must not exceed E * T).  Waits for `stream`. */
int lg_distill_rtrain_step_losses(lg_distill_rtrain* trainer, float* losses_host, int64_t count, void* stream);

/* The carry (running == 0) or the running state after the last step run (running != 0): h (L, N, H) and, for an LSTM, c (c may be NULL).  h and c
 * may be HOST or device memory (the copy finds out): the Python layer hands the carry to the policy's live memory without leaving the device.
 * get_carry returns N (0: no rows yet) and copies only if h is not NULL and capacity_rows >= N.  set_carry installs both the carry and the running
 * state for N rows; reset_carry forgets them (the next call starts from zeros, with any N).  get_carry and set_carry wait for `stream`. */
int64_t lg_distill_rtrain_get_carry(lg_distill_rtrain* trainer, float* h, float* c, int64_t capacity_rows, int32_t running, void* stream);
int lg_distill_rtrain_set_carry(lg_distill_rtrain* trainer, const float* h, const float* c, int64_t N, void* stream);
int lg_distill_rtrain_reset_carry(lg_distill_rtrain* trainer, void* stream);

/* Checkpoints, as the calls of lgdistill.h: all HOST, flat as above; any pointer of get_state may be NULL.  set_state also rewrites the images. */
int lg_distill_rtrain_get_parameters(lg_distill_rtrain* trainer, float* parameters_host, void* stream);
int lg_distill_rtrain_get_state(lg_distill_rtrain* trainer, float* parameters_host, float* exp_avg_host, float* exp_avg_sq_host, int64_t* step_host,
                                double* learning_rate_host, void* stream);
int lg_distill_rtrain_set_state(lg_distill_rtrain* trainer, const float* parameters_host, const float* exp_avg_host, const float* exp_avg_sq_host,
                                int64_t step, double learning_rate, void* stream);
int lg_distill_rtrain_set_learning_rate(lg_distill_rtrain* trainer, double learning_rate, void* stream);

#ifdef __cplusplus
}
#endif
#endif
