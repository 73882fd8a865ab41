/* lgtrain_symmetry.h — C ABI of PPO.update with the symmetry option of the vendored rsl_rl (algorithms/ppo.py:234-370): symmetric data augmentation
 * and the mirror loss, for the feed-forward ActorCritic.  Same library, same conventions and the same row / hyper-parameter structs as lgtrain.h.
 *
 * The augmentation function is handed over as tables: it must be a signed permutation of columns, out_k[:, c] = sign_k[c] * in[:, perm_k[c]], for each
 * of its K blocks (block 0: the identity, the original rows).  The tables are applied while the kernels stage rows; no augmented batch is ever
 * materialised.  With B the rows of a mini-batch, logical row k * B + j is block k of mini-batch row j.
 *   use_data_augmentation: the PPO losses run on the K * B rows (row k * B + j carries the transformed observations and actions of row j and row j's
 *     old log-prob, value, advantage and return); their means divide by K * B.  Entropy and KL use the first B rows only.
 *   otherwise: the PPO losses and the critic run on the B original rows; the actor also runs on the (K - 1) * B transformed rows, for the mirror term only.
 *   symmetry loss = mean over rows i >= B and actions of (mu_i - T_k(mu_j))^2, the target detached.  With use_mirror_loss, mirror_loss_coeff times it joins
 *     the loss; without, it is only reported.
 * Equal inputs give equal bits: no atomics anywhere; every sum has a fixed order. */
#ifndef LGTRAIN_SYMMETRY_H
#define LGTRAIN_SYMMETRY_H
#include <stdint.h>
#include "lgtrain.h"
#ifdef __cplusplus
extern "C" {
#endif

#define LG_PPO_SYM_MAX_BLOCKS 4      /* K at most: the original and three transformed copies */

typedef struct lg_ppo_sym lg_ppo_sym;

/* HOST.  perm: (num_blocks, width) int32, row-major; sign: the same shape, float32, every entry +1 or -1.  The critic tables are separate because the
 * critic's observations may have another layout. */
typedef struct lg_ppo_sym_tables {
  int32_t num_blocks;
  int32_t observation_width;
  int32_t critic_observation_width;
  int32_t action_width;
  const int32_t* observation_perm;
  const float* observation_sign;
  const int32_t* critic_observation_perm;
  const float* critic_observation_sign;
  const int32_t* action_perm;
  const float* action_sign;
} lg_ppo_sym_tables;

typedef struct lg_ppo_sym_config {
  int32_t use_data_augmentation;
  int32_t use_mirror_loss;
  float mirror_loss_coeff;
} lg_ppo_sym_config;

/* lg_ppo_stats and the mean of the symmetry loss over the update's optimiser steps (device memory, float64). */
typedef struct lg_ppo_sym_stats {
  double value_function;
  double surrogate;
  double entropy;
  double kl;
  double learning_rate;
  double symmetry;
} lg_ppo_sym_stats;

/* As lg_ppo_create, with the tables and the option.  max_rows counts mini-batch rows B; the workspaces hold num_blocks * max_rows rows.  Refused as
 * lg_ppo_create, and: NULL tables or config, num_blocks < 2 or > LG_PPO_SYM_MAX_BLOCKS, a table width that is not the network's, an index outside
 * [0, width), a sign that is not +1 or -1, a block 0 that is not the identity, a mirror_loss_coeff that is not finite. */
lg_ppo_sym* lg_ppo_sym_create(lg_mlp* actor, lg_mlp* critic, const float* const* actor_weights, const float* const* actor_biases,
                              const float* const* critic_weights, const float* const* critic_biases, const float* std_host, int32_t noise_std_type,
                              double learning_rate, int64_t max_rows, float* std_device, const lg_ppo_sym_tables* tables, const lg_ppo_sym_config* config);
void lg_ppo_sym_destroy(lg_ppo_sym* ppo);

/* As lg_ppo_minibatch / lg_ppo_update: count and R count ORIGINAL rows. */
int lg_ppo_sym_minibatch(lg_ppo_sym* ppo, const lg_ppo_rows* rows, const int64_t* indices, int64_t count, const lg_ppo_hyper* hyper, void* stream);
int lg_ppo_sym_update(lg_ppo_sym* ppo, const lg_ppo_rows* rows, int64_t R, const int64_t* indices, int32_t num_mini_batches, int32_t num_learning_epochs,
                      const lg_ppo_hyper* hyper, lg_ppo_sym_stats* stats, void* stream);

int64_t lg_ppo_sym_parameter_count(lg_ppo_sym* ppo);

/* As lg_ppo_gradients; symmetry_loss_host (HOST, 1 float, may be NULL): the last mini-batch's symmetry loss. */
int lg_ppo_sym_gradients(lg_ppo_sym* ppo, float* gradients_host, float* global_norm_host, float* loss_means_host, float* symmetry_loss_host, void* stream);

/* The outputs of the last mini-batch's forward pass (HOST): action means (num_blocks * count, A) in logical row order, and values: (num_blocks * count)
 * with use_data_augmentation, else (count) -- the critic does not see transformed rows then.  Either may be NULL.  Waits for `stream`. */
int lg_ppo_sym_forward_outputs(lg_ppo_sym* ppo, float* action_mean_host, float* values_host, void* stream);

int lg_ppo_sym_get_parameters(lg_ppo_sym* ppo, float* parameters_host, void* stream);
int lg_ppo_sym_get_state(lg_ppo_sym* ppo, float* parameters_host, float* exp_avg_host, float* exp_avg_sq_host, int64_t* step_host, double* learning_rate_host,
                         void* stream);
int lg_ppo_sym_set_state(lg_ppo_sym* ppo, const float* parameters_host, const float* exp_avg_host, const float* exp_avg_sq_host, int64_t step,
                         double learning_rate, void* stream);
int lg_ppo_sym_set_learning_rate(lg_ppo_sym* ppo, double learning_rate, void* stream);

#ifdef __cplusplus
}
#endif
#endif
