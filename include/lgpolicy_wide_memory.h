/* lgpolicy_wide_memory.h — the wide observation row in front of a memory: lg_rnn_create_wide.  Part of lgpolicy_wide.h, which includes it; same
 * library, same error channel (lg_mlp_last_error), same handle type lg_rnn. */
#ifndef LGPOLICY_WIDE_MEMORY_H
#define LGPOLICY_WIDE_MEMORY_H
#include "lgpolicy.h"
#ifdef __cplusplus
extern "C" {
#endif

/* lg_rnn_create with an input row of up to LG_RNN_MAX_INPUT columns; hidden stays 1..512 and layers above the first read `hidden` columns as ever.
 * For input <= 512 the handle is lg_rnn_create's: same images, same kernels, same bits (lg_rnn_create itself keeps refusing 513).  Layer 0 of a
 * handle with more inputs is two launches.  The input projection x W_ih^T runs first, the row staged in slabs of 512 columns, every output ONE
 * k-ascending fp32 chain over blocks of 16 inputs (the order the one-launch layer walks the x part of [x ; h]), stored unrounded in a workspace the
 * handle owns (n x gates x hidden padded to 16 floats; allocated at the first step, regrown when n grows, never shrunk).  The step then starts its
 * accumulators from that row and goes on over the h blocks: the narrow chain, cut at the x / h boundary.  So a wide memory whose w_ih is zero from
 * column 512 on gives the bits of the 512-input memory, and the slab size changes nothing.  Every entry point that steps a memory takes such a handle:
 * lg_rnn_step, lg_policy_act_recurrent, lg_distill_act_recurrent, lg_collect_rollout_recurrent, lg_collect_distillation_recurrent, the
 * lg_runner_collect* family (lg_runner_collect_sensors included), and lg_ppo_recurrent_create trains it; a pair of memories may be wide, narrow or
 * mixed.  lg_distill_rtrain_create, lg_estimator_train_create and lg_estimator_step refuse a wide memory by name.
 * NULL + "lg_rnn_create_wide: <which width, and its bound>" in lg_mlp_last_error(NULL) otherwise, with nothing allocated; the argument checks come
 * before the device check.
 * Diagnostic only: with LG_RNN_FORCE_WIDE=1 in the environment when this function is called, a memory of 512 inputs or fewer takes the wide
 * kernels too (tests compare its bits with lg_rnn_create's); any value but 0 or 1 is refused, the message naming the variable and the value. */
#define LG_RNN_MAX_INPUT 2048
lg_rnn* lg_rnn_create_wide(int32_t type, int32_t num_layers, int32_t input, int32_t hidden, const float* const* w_ih, const float* const* w_hh,
                           const float* const* b_ih, const float* const* b_hh, int device_id);

/* The two device images of a wide memory's layer 0, a pure host function (no device): tiled_x[((c * (nbx + 1) + b) * G + g) * 64 + lane][s] =
 * w_ih[g * hidden + 16 c + (lane & 15)][16 b + 4 s + (lane >> 4)] over nbx = ceil(input / 16) blocks and one more, all-zero, block per chunk c of 16
 * hidden units; tiled_h the same over w_hh with ceil(hidden / 16) + 1 blocks; zero wherever the index leaves the matrix.  G = 4 (LSTM: i f g o) or
 * 3 (GRU: r z n).  Returns the float count of tiled_x and stores tiled_h's in *count_h; either buffer may be NULL (sizes only).  A negative status
 * with a message on a bad argument. */
int64_t lg_rnn_tile_weights_wide(int32_t type, int32_t input, int32_t hidden, const float* w_ih, const float* w_hh, float* tiled_x, float* tiled_h,
                                 int64_t* count_h);

#ifdef __cplusplus
}
#endif
#endif
