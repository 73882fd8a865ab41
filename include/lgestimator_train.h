/* lgestimator_train.h — C ABI of the training side of the terrain estimator: EstimatorDistillation.update of the vendored rsl_rl
 * (algorithms/distillation.py:277-332, through runners/terrain_estimator_runner.py) on the device.  The trainer sits on the FOUR handles of an
 * estimator that already exists (lgpolicy.h: depth encoder, combination layer, memory, decoder); forward with saved maps, the loss, the backward pass
 * through the decoder, the memory (truncated BPTT), the combination layer and the convolutions, the weight gradients, the optional grad-norm clip and
 * Adam run on the device and rewrite the images lg_estimator_step and lg_conv_encoder_forward read.  Same library and conventions as lgdistill.h:
 * device pointers unless marked HOST, asynchronous on the caller's hipStream_t unless a call copies to the HOST, 0 / negative status, and ONE error
 * channel: every refusal leaves "<entry point>: <reason>" in the thread's message (lg_mlp_last_error of lgpolicy.h) and launches nothing.
 *
 * An update walks E * T steps, epoch-major.  Step k reads time index t_k = k mod T of depth_images (T, N, h, w), proprio (T, N, P) and targets
 * (T, N, R); its loss l_k = loss_fn(estimator(depth[t_k], proprio[t_k]), target[t_k]) is an fp32 mean over N * R elements.  Every G = gradient_length
 * consecutive steps form a group, which may straddle an epoch boundary: one optimiser step on the gradient of the SUM of the group's losses.  The
 * trailing (E * T) mod G steps run forward only with the final weights; they count in the reported mean and advance the memory.
 *
 * The memory.  Gradients flow through the memory inside a group (truncated BPTT); a group's first step enters with the state the step before it left,
 * as a constant.  A step with t_k = 0 (the first of every epoch) enters with the CARRY as a constant: the state the last update ended with, zeros
 * before the first -- every epoch re-seeds from the carry the update started with, not from the previous epoch's end (distillation.py:284-285).
 * After an update the carry is the state after its last step.  The trainer owns the carry (L, N, H) (+ c for an LSTM) and the running state; the
 * live inference state of the estimator's lg_rnn callers is not touched.  use_dones != 0: a row with dones[t] != 0 enters step t + 1 with zero state
 * and no gradient crosses (the reference's storage holds all-zero dones: use_dones = 0 is its behaviour).
 *
 * Parameters: one flat fp32 vector in the module's state_dict() order, each tensor in torch's layout: depth_encoder.{0,2,4,6,10,12} (weight, bias),
 * combination_mlp.0 (weight, bias), memory.rnn.{weight_ih, weight_hh, bias_ih, bias_hh}_l{l} per layer, decoder.* (weight, bias).
 *
 * Workspace.  The saved maps of a group are KEPT (nothing is recomputed in the backward pass): per row of a group (a row = one env of one step), for
 * an h x w image with conv maps of p1, p2, p3, p3 pixels (28 x 56: 392, 98, 28, 28), 32 p1 + 64 p2 + 128 p3 + 64 p3 floats of maps
 * (12 544 + 6 272 + 3 584 + 1 792), the two ping-pong delta buffers max(32 p1, 128 p3) + max(64 p2, 64 p3) (12 544 + 6 272), 2 x 1024 + 2 x 128 floats
 * around the pooling and the first linear layer, and the rows of the combination layer, the memory (gates, states, gate derivatives) and the decoder.
 * At 28 x 56 with a GRU of 256 and the decoder 128-64-81 that is about 50 000 floats per row: 4096 envs x G = 15 take 12.3 GB, of which the maps are
 * 5.9 GB (derived).  The slab partials of the weight gradients add ceil(rows x pixels / slab) x C_out x (K + 1) floats per convolution and one slab
 * per 256 rows of every dense matrix.  workspace_bytes reports what was allocated: 13.1 GB for that shape (measured).
 *
 * Equal inputs give equal bits: no atomics anywhere; every sum has a fixed order. */
#ifndef LGESTIMATOR_TRAIN_H
#define LGESTIMATOR_TRAIN_H
#include <stdint.h>
#include "lgpolicy.h"
#ifdef __cplusplus
extern "C" {
#endif

enum lg_estimator_loss { LG_EST_LOSS_MSE = 0, LG_EST_LOSS_HUBER = 1, LG_EST_LOSS_L1 = 2 };   /* huber: delta = 1; l1: a zero difference has gradient 0 */

typedef struct lg_estimator_train lg_estimator_train;

typedef struct lg_estimator_train_hyper {
  int32_t loss_type;                 /* lg_estimator_loss */
  float max_grad_norm;               /* <= 0: no clip (None or 0 in the reference); the norm is computed and reported either way */
  int32_t use_dones;                 /* != 0: the rows' dones reset the memory inside an update */
} lg_estimator_train_hyper;

/* HOST pointers to the module's tensors in torch's layout.  encoder_*[6]: depth_encoder.{0,2,4,6,10,12}; memory_*[num_layers]; decoder_*[layers of
 * the decoder handle]. */
typedef struct lg_estimator_train_params {
  const float* const* encoder_weights; const float* const* encoder_biases;
  const float* combine_weight; const float* combine_bias;
  const float* const* memory_w_ih; const float* const* memory_w_hh; const float* const* memory_b_ih; const float* const* memory_b_hh;
  const float* const* decoder_weights; const float* const* decoder_biases;
} lg_estimator_train_params;

/* What an update reports (device memory, float64): the mean of the E * T step losses (each an fp32 mean, summed as float64 in step order), the number
 * of optimiser steps, and the global gradient norm of the last one (before the clip; unchanged if none was taken). */
typedef struct lg_estimator_train_stats {
  double estimation;
  double optimizer_steps;
  double grad_norm;
} lg_estimator_train_stats;

/* A trainer over the estimator's four handles, which must outlive it.  The HOST parameters become the fp32 masters Adam updates, and the create call
 * rewrites every device image from them.  Moments, step count and carry start at zero.  max_rows: the largest G * N a group may have.  Refused: a
 * NULL handle or pointer, max_rows < 1, a learning rate that is not > 0, an encoder that is not LG_PREC_F32 (lg_estimator_bf16train_create of
 * lgestimator_train_bf16.h trains it; or train fp32, then build a bf16 estimator from the trained parameters), stages whose widths do not chain or that live on different devices. */
lg_estimator_train* lg_estimator_train_create(lg_conv_encoder* encoder, lg_mlp* combine, lg_rnn* memory, lg_mlp* decoder, const lg_estimator_train_params* params,
                                              double learning_rate, int64_t max_rows);
void lg_estimator_train_destroy(lg_estimator_train* trainer);

/* num_steps consecutive steps from step first_step of the sequence (step s reads time index (first_step + s) mod T); train != 0: one optimiser step
 * on the sum of their losses, else forward and losses only (the remainder of an update).  depth (T, N, h, w), proprio (T, N, P), targets (T, N, R),
 * dones (T, N; may be NULL unless use_dones): time-major, contiguous.  A step with time index 0 enters with the carry, every other first step with
 * the running state; the running state is left after the last step, the carry is not written.  Refused: NULL handle or pointer, T, N or num_steps
 * < 1, first_step < 0, num_steps * N > max_rows, an unknown loss type, an N that is not the carry's (reset_carry first). */
int lg_estimator_train_group(lg_estimator_train* trainer, const float* depth, const float* proprio, const float* targets, const float* dones, int64_t T,
                             int64_t N, int64_t first_step, int64_t num_steps, int32_t train, const lg_estimator_train_hyper* hyper, void* stream);

/* EstimatorDistillation.update: floor(E * T / G) groups, the remainder forward-only, then carry := the running state.  Nothing is synchronised;
 * stats (device, may be NULL) is written by the last kernel.  Refused as the group call, and for num_learning_epochs or gradient_length < 1 or
 * gradient_length * N > max_rows. */
int lg_estimator_train_update(lg_estimator_train* trainer, const float* depth, const float* proprio, const float* targets, const float* dones, int64_t T,
                              int64_t N, int32_t num_learning_epochs, int32_t gradient_length, const lg_estimator_train_hyper* hyper,
                              lg_estimator_train_stats* stats, void* stream);

/* Number of floats of the flat parameter vector; bytes of device memory the trainer holds; rows (env, output pixel) per slab of the convolutions'
 * weight-gradient pass. */
int64_t lg_estimator_train_parameter_count(lg_estimator_train* trainer);
int64_t lg_estimator_train_workspace_bytes(lg_estimator_train* trainer);
int32_t lg_estimator_train_wgrad_slab_rows(void);

/* The last group's gradients BEFORE the clip (HOST, flat as above), its global norm, and its per-step losses (HOST, capacity floats; LG_ERR_INVALID
 * if the group had more steps).  Any of the three may be NULL.  Waits for `stream`. */
int lg_estimator_train_gradients(lg_estimator_train* trainer, float* gradients_host, float* global_norm_host, float* step_losses_host, int64_t capacity,
                                 void* stream);
/* The predictions (rows, R) of the last group call's forward pass, step-major (HOST).  Waits for `stream`. */
int lg_estimator_train_forward_outputs(lg_estimator_train* trainer, float* predictions_host, void* stream);
/* The E * T step losses of the last update (HOST, count floats; count must not exceed E * T).  Waits for `stream`. */
int lg_estimator_train_step_losses(lg_estimator_train* trainer, float* losses_host, int64_t count, void* stream);

/* The carry (running == 0) or the running state after the last step run (running != 0): h (L, N, H) and, for an LSTM, c (HOST; c may be NULL).
 * get_carry returns N (0: no rows yet) and copies only if h_host is not NULL and capacity_rows >= N.  set_carry installs both the carry and the
 * running state for N rows; reset_carry forgets them (the next call starts from zeros, with any N). */
int64_t lg_estimator_train_get_carry(lg_estimator_train* trainer, float* h_host, float* c_host, int64_t capacity_rows, int32_t running, void* stream);
int lg_estimator_train_set_carry(lg_estimator_train* trainer, const float* h_host, const float* c_host, int64_t N, void* stream);
int lg_estimator_train_reset_carry(lg_estimator_train* trainer, void* stream);

/* Checkpoints, as the calls of lgdistill.h: all HOST, flat as above; any pointer of get_state may be NULL.  set_state also rewrites the images. */
int lg_estimator_train_get_parameters(lg_estimator_train* trainer, float* parameters_host, void* stream);
int lg_estimator_train_get_state(lg_estimator_train* trainer, float* parameters_host, float* exp_avg_host, float* exp_avg_sq_host, int64_t* step_host,
                                 double* learning_rate_host, void* stream);
int lg_estimator_train_set_state(lg_estimator_train* trainer, const float* parameters_host, const float* exp_avg_host, const float* exp_avg_sq_host,
                                 int64_t step, double learning_rate, void* stream);
int lg_estimator_train_set_learning_rate(lg_estimator_train* trainer, double learning_rate, void* stream);

#ifdef __cplusplus
}
#endif
#endif
