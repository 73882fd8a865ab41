/* lgtrain.h — C ABI of the training side of PPO: PPO.update of the vendored rsl_rl (algorithms/ppo.py:197-438, mini-batches as
 * storage/rollout_storage.py:184-243) for the feed-forward ActorCritic, on the fp32 matrix cores.  Forward with saved activations, the clipped
 * losses, the backward data pass, the weight gradients, global grad-norm clipping and Adam all run on the device; the weights stay there and are
 * updated in place, in the tiled images the acts and collectors of lgpolicy.h read.  Same library (extended_legged_gym_amd/csrc/liblgstep.so) and
 * same conventions as lgpolicy.h: device pointers unless marked HOST, asynchronous on the caller's hipStream_t unless a call copies to the HOST,
 * 0 / negative status as in lgstep.h, and ONE error channel: every refusal leaves "<entry point>: <reason>" in the thread's message (read with the
 * last-error call of lgpolicy.h) and launches nothing.
 *
 * Not built here, refused by the Python layer: recurrent policies (lgtrain_recurrent.h), symmetry_cfg (lgtrain_symmetry.h), RND, normalize_advantage_per_mini_batch, multi-GPU reduction.
 * Equal inputs give equal bits: no atomics anywhere; every sum has a fixed order. */
#ifndef LGTRAIN_H
#define LGTRAIN_H
#include <stdint.h>
#include "lgpolicy.h"
#ifdef __cplusplus
extern "C" {
#endif

enum lg_noise_std_type { LG_STD_SCALAR = 0, LG_STD_LOG = 1 };          /* ActorCritic(noise_std_type=...): the parameter is std, or log_std */
enum lg_lr_schedule { LG_SCHEDULE_FIXED = 0, LG_SCHEDULE_ADAPTIVE = 1 };

typedef struct lg_ppo lg_ppo;

/* The flattened (R, .) rows of a rollout, as RolloutStorage.mini_batch_generator flattens them (rollout_storage.py:193-208).  critic_observations
 * may equal observations.  values, returns, advantages, actions_log_prob: (R, 1); actions, mu, sigma: (R, A). */
typedef struct lg_ppo_rows {
  const float* observations;
  const float* critic_observations;
  const float* actions;
  const float* values;
  const float* returns;
  const float* advantages;
  const float* actions_log_prob;
  const float* mu;
  const float* sigma;
} lg_ppo_rows;

typedef struct lg_ppo_hyper {
  float clip_param;
  float value_loss_coef;
  float entropy_coef;
  int32_t use_clipped_value_loss;
  float max_grad_norm;
  int32_t schedule;                  /* lg_lr_schedule */
  double desired_kl;                 /* float64: the thresholds 2 desired_kl and desired_kl / 2 are the reference's Python doubles */
} lg_ppo_hyper;

/* What an update reports (device memory, float64): the means over its E * M optimiser steps of the value loss, the surrogate loss, the entropy
 * and the KL to the collection policy (ppo.py:403-417), and the learning rate after the last step. */
typedef struct lg_ppo_stats {
  double value_function;
  double surrogate;
  double entropy;
  double kl;
  double learning_rate;
} lg_ppo_stats;

/* A trainer over two networks that already exist.  Parameters are passed once more as HOST pointers in torch's layout (weights[l]: (out, in)
 * row-major; biases[l]: (out)); they become the fp32 master copy Adam updates.  std_host (A): the std parameter, or log_std for LG_STD_LOG.
 * std_device (A): the device vector the acts read; every step rewrites it (std, or exp(log_std)).  The create call writes both networks' tiled
 * images and std_device from the masters, so they agree by construction; it zeroes the moments and the step count and allocates workspaces for
 * mini-batches of up to max_rows rows.  The trainer writes into the two networks' device buffers at every step: both networks must outlive it
 * (destroy the trainer first).  Refused: a learning rate that is not > 0, NULL handles or pointers, max_rows < 1, networks on different devices, a critic whose output is
 * not 1 wide, an actor with more than 32 actions, an unknown std type, a network whose output activation is set. */
lg_ppo* lg_ppo_create(lg_mlp* actor, lg_mlp* critic, const float* const* actor_weights, const float* const* actor_biases,
                      const float* const* critic_weights, const float* const* critic_biases, const float* std_host, int32_t noise_std_type,
                      double learning_rate, int64_t max_rows, float* std_device);
void lg_ppo_destroy(lg_ppo* ppo);

/* One optimiser step (the body of the loop ppo.py:219-411) on the rows rows[indices[0 .. count)].  indices: int64, device; they are NOT
 * range-checked on the device.  Refused: NULL handle or pointer, count <= 0, count > max_rows, an unknown schedule. */
int lg_ppo_minibatch(lg_ppo* ppo, const lg_ppo_rows* rows, const int64_t* indices, int64_t count, const lg_ppo_hyper* hyper, void* stream);

/* PPO.update: num_learning_epochs passes over num_mini_batches slices of `indices` (a permutation of [0, R), int64, device; the same one in
 * every epoch, as rollout_storage.py:189-217), each slice R / num_mini_batches rows (integer division) and one lg_ppo_minibatch.  Nothing is
 * synchronised: the whole update is enqueued.  stats (device, may be NULL) is written by the last kernel.  Refused as lg_ppo_minibatch, and
 * for num_mini_batches < 1, num_learning_epochs < 1 or R / num_mini_batches == 0. */
int lg_ppo_update(lg_ppo* ppo, const lg_ppo_rows* rows, int64_t R, const int64_t* indices, int32_t num_mini_batches, int32_t num_learning_epochs,
                  const lg_ppo_hyper* hyper, lg_ppo_stats* stats, void* stream);

/* Number of floats of the flat parameter vector: actor (W0, b0, W1, b1, ...), critic likewise, then std / log_std -- each tensor in torch's
 * layout, the order of ActorCritic.parameters(). */
int64_t lg_ppo_parameter_count(lg_ppo* ppo);

/* The gradients of the last mini-batch BEFORE the norm clip (HOST, flat as above), its global norm, and its four loss means (HOST, 4 floats:
 * surrogate, value, entropy, KL).  Any of the three may be NULL.  Waits for `stream`. */
int lg_ppo_gradients(lg_ppo* ppo, float* gradients_host, float* global_norm_host, float* loss_means_host, void* stream);

/* The outputs of the last mini-batch's forward pass (HOST): action means (count, A) and values (count), in mini-batch order.  Either may be NULL.
 * Waits for `stream`. */
int lg_ppo_forward_outputs(lg_ppo* ppo, float* action_mean_host, float* values_host, void* stream);

/* Checkpoints.  All HOST, flat as above; any pointer of get_state may be NULL.  exp_avg / exp_avg_sq: Adam's moments; step: optimiser steps taken.
 * set_state also rewrites the tiled images and std_device from the new masters.  Wait for `stream`. */
int lg_ppo_get_parameters(lg_ppo* ppo, float* parameters_host, void* stream);
int lg_ppo_get_state(lg_ppo* ppo, float* parameters_host, float* exp_avg_host, float* exp_avg_sq_host, int64_t* step_host, double* learning_rate_host,
                     void* stream);
int lg_ppo_set_state(lg_ppo* ppo, const float* parameters_host, const float* exp_avg_host, const float* exp_avg_sq_host, int64_t step,
                     double learning_rate, void* stream);
int lg_ppo_set_learning_rate(lg_ppo* ppo, double learning_rate, void* stream);

/* Rows of one batch slab of the weight-gradient pass (the batch dimension is split into slabs of this size, reduced in slab order). */
int32_t lg_ppo_wgrad_slab_rows(void);

#ifdef __cplusplus
}
#endif
#endif
