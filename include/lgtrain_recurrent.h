/* lgtrain_recurrent.h — C ABI of PPO.update for the recurrent actor-critic (vendored rsl_rl: algorithms/ppo.py:197-438 with the mini-batches of
 * storage/rollout_storage.py:246-316 and modules/actor_critic_recurrent.py:62-85): backpropagation through time through the nn.LSTM / nn.GRU
 * memory in front of each MLP, on the fp32 matrix cores.  Same library and conventions as lgtrain.h: device pointers unless marked HOST,
 * asynchronous on the caller's hipStream_t unless a call copies to the HOST, 0 / negative status as in lgstep.h, ONE error channel (every refusal
 * leaves "<entry point>: <reason>" in the thread's message, read with the last-error call of lgpolicy.h, and launches nothing).  No atomics: every
 * sum has a fixed order, equal inputs give equal bits.
 *
 * The formulation.  The reference takes mini-batches as env slices over all T steps, splits every env's column at its dones, pads the pieces,
 * starts each piece from the hidden row saved at its first step and runs the memory over the padded block; its losses are plain means over the
 * T * count rows.  Here the same arithmetic runs without the padding: the slice is walked in time order, and row j enters step t with the saved
 * hidden row hidden[t][:, env0 + j] when t == 0 or dones[t - 1][env0 + j] != 0, otherwise with its own state after step t - 1; in the backward
 * pass no gradient crosses from step t to step t - 1 for such a row.  Mini-batch row i = t * count + j is rollout row t * N + env0 + j (the
 * reference's (T, count) flatten).
 *
 * One optimiser step: T x layers forward launches (both memories side by side) that save their gates, the MLPs' forward, loss and backward of
 * lgtrain.h over the T * count rows plus dL/d(input) of their first layers, T x layers backward launches (gate derivative, then
 * [dx ; dh_prev] = D Wcat from transposed tilings), ONE weight-gradient pass over all T * count rows (weight_ih + bias_ih with (D_ih, x),
 * weight_hh + bias_hh with (D_hh, h_in)), the norm, Adam, and the rewrite of every tiled image -- the lg_rnn images included, bit-equal to
 * lg_rnn_tile_weights of the masters.
 *
 * Workspace per mini-batch row (floats), H the hidden width, G = 4 (LSTM) or 3 (GRU), per memory and layer: the saved gates 4 H, the entering and
 * the new h 2 H (+ 2 H for an LSTM's cell), dL/dh' from above H, the gate derivatives G H (twice for a GRU, whose hidden side differs in the n gate)
 * and the two ping-pong carries 2 H (+ 2 H for the cell): 17 H for an LSTM, 15 H for a GRU -- the saved gates and their derivatives dominate.  On
 * top, the MLPs' 2 x (sum of their layer widths) of lgtrain.h, 2 floats for the row index, and per weight-gradient slab (the slab size of
 * lgtrain.h) one partial of every weight matrix.  lg_ppo_recurrent_workspace_bytes reports the total of a trainer. */
#ifndef LGTRAIN_RECURRENT_H
#define LGTRAIN_RECURRENT_H
#include <stdint.h>
#include "lgtrain.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct lg_ppo_recurrent lg_ppo_recurrent;

/* HOST: the parameters of an ActorCriticRecurrent in torch's layout, and the shapes they were taken from.  mem_?_w_ih[l]: memory_?.rnn.weight_ih_l{l}
 * (G hidden, input or hidden); w_hh[l]: (G hidden, hidden); b_ih[l] / b_hh[l]: (G hidden).  actor / critic lists as lg_ppo_create.  std: the std
 * parameter (A), or log_std for LG_STD_LOG. */
typedef struct lg_ppo_recurrent_params {
  int32_t rnn_type;                  /* lg_rnn_type */
  int32_t num_layers;
  int32_t input_a, hidden_a;         /* memory_a: observation width, hidden width */
  int32_t input_c, hidden_c;
  const float* const* mem_a_w_ih;
  const float* const* mem_a_w_hh;
  const float* const* mem_a_b_ih;
  const float* const* mem_a_b_hh;
  const float* const* mem_c_w_ih;
  const float* const* mem_c_w_hh;
  const float* const* mem_c_b_ih;
  const float* const* mem_c_b_hh;
  const float* const* actor_weights;
  const float* const* actor_biases;
  const float* const* critic_weights;
  const float* const* critic_biases;
  const float* std;
} lg_ppo_recurrent_params;

/* A trainer over two memories and two MLPs that already exist.  The HOST parameters become the fp32 masters; the create call writes EVERY tiled
 * image from them -- the MLPs', std_device, and the lg_rnn images in the layout lg_rnn_tile_weights documents -- so the acts and the trainer agree
 * by construction.  Workspaces hold mini-batches of up to max_rows = T * count rows.  The four handles must outlive the trainer.
 * Refused: NULL handles or pointers; a type, depth or width in `params` that is not the handle's (LSTM against GRU, widths that disagree); memories
 * of different type or depth; an MLP whose input is not its memory's hidden width; handles on different devices; and whatever lg_ppo_create refuses. */
lg_ppo_recurrent* lg_ppo_recurrent_create(lg_rnn* mem_a, lg_mlp* actor, lg_rnn* mem_c, lg_mlp* critic, const lg_ppo_recurrent_params* params,
                                          int32_t noise_std_type, double learning_rate, int64_t max_rows, float* std_device);
void lg_ppo_recurrent_destroy(lg_ppo_recurrent* ppo);

/* One optimiser step on the env slice [env0, env0 + count) of a (T, N, .) rollout.  rows: lg_ppo_rows pointing at the UNFLATTENED rollout
 * ((T, N, O) observations, ...); hidden: the (T, num_layers, N, hidden) rows lg_collect_rollout_recurrent keeps (c_a / c_c NULL for a GRU);
 * dones: (T, N).  Refused: NULL handle or pointer, T < 1, count < 1, env0 < 0, env0 + count > N, T * count > max_rows, an unknown schedule. */
int lg_ppo_recurrent_minibatch(lg_ppo_recurrent* ppo, const lg_ppo_rows* rows, const lg_rollout_hidden* hidden, const float* dones, int32_t T, int64_t N,
                               int64_t env0, int64_t count, const lg_ppo_hyper* hyper, void* stream);

/* PPO.update: num_learning_epochs passes over num_mini_batches slices [i (N / M), (i + 1) (N / M)) (integer division; the envs beyond M (N / M) are
 * unused and every epoch takes the same slices, as rollout_storage.py:246-316).  Nothing is synchronised; stats (device, may be NULL) is written
 * by the last kernel.  Refused as lg_ppo_recurrent_minibatch, and for num_mini_batches < 1, num_learning_epochs < 1 or N / num_mini_batches == 0. */
int lg_ppo_recurrent_update(lg_ppo_recurrent* ppo, const lg_ppo_rows* rows, const lg_rollout_hidden* hidden, const float* dones, int32_t T, int64_t N,
                            int32_t num_mini_batches, int32_t num_learning_epochs, const lg_ppo_hyper* hyper, lg_ppo_stats* stats, void* stream);

/* Number of floats of the flat parameter vector.  Its order is fixed: actor (W0, b0, W1, b1, ...), critic likewise, memory_a per layer
 * (weight_ih, weight_hh, bias_ih, bias_hh), memory_c likewise, then std / log_std -- each tensor in torch's layout. */
int64_t lg_ppo_recurrent_parameter_count(lg_ppo_recurrent* ppo);
/* Bytes of device memory the trainer allocated (workspaces, masters, moments, tilings). */
int64_t lg_ppo_recurrent_workspace_bytes(lg_ppo_recurrent* ppo);

/* As lg_ppo_gradients / lg_ppo_forward_outputs: the last mini-batch's gradients BEFORE the clip (HOST, flat as above), norm and four loss means
 * (surrogate, value, entropy, KL); its action means (T * count, A) and values (T * count) in mini-batch order.  Wait for `stream`. */
int lg_ppo_recurrent_gradients(lg_ppo_recurrent* ppo, float* gradients_host, float* global_norm_host, float* loss_means_host, void* stream);
int lg_ppo_recurrent_forward_outputs(lg_ppo_recurrent* ppo, float* action_mean_host, float* values_host, void* stream);

/* Checkpoints, as lgtrain.h.  set_state rewrites every tiled image from the new masters. */
int lg_ppo_recurrent_get_parameters(lg_ppo_recurrent* ppo, float* parameters_host, void* stream);
int lg_ppo_recurrent_get_state(lg_ppo_recurrent* ppo, float* parameters_host, float* exp_avg_host, float* exp_avg_sq_host, int64_t* step_host,
                               double* learning_rate_host, void* stream);
int lg_ppo_recurrent_set_state(lg_ppo_recurrent* ppo, const float* parameters_host, const float* exp_avg_host, const float* exp_avg_sq_host, int64_t step,
                               double learning_rate, void* stream);
int lg_ppo_recurrent_set_learning_rate(lg_ppo_recurrent* ppo, double learning_rate, void* stream);

/* The device images of one memory layer as the acts read them (HOST): memory 0 (actor's) or 1, the tiled weights (lg_rnn_tile_weights' count of
 * floats) and the tiled bias (4 x hidden rounded up to 16).  Either may be NULL.  Waits for `stream`. */
int lg_ppo_recurrent_get_images(lg_ppo_recurrent* ppo, int32_t memory, int32_t layer, float* tiled_weights_host, float* tiled_bias_host, void* stream);

#ifdef __cplusplus
}
#endif
#endif
