/* lgestimator_train_bf16.h — C ABI of the opt-in bf16 training of the terrain estimator's depth encoder.  The trainer is an lg_estimator_train
 * (lgestimator_train.h): every lg_estimator_train_* call works on it unchanged.  What differs is the function it differentiates and the kernels of
 * the encoder's backward pass.
 *
 * Write R(v) for v rounded to bf16, nearest even.  The trainer differentiates the function an LG_PREC_BF16 estimator computes: the image and the
 * encoder's six weight tensors go through R, the outputs of stages 1-6 (conv 1-4, pool + flatten, linear 1) go through R; biases, bias add,
 * activation and accumulation are fp32; the features, the combination layer, the memory and the decoder are fp32, as lg_estimator_step runs them.
 * Rounding is straight-through (dR/dv = 1); an activation's derivative is taken from its stored, rounded output.  Master parameters, gradients, their
 * slab partials and reductions, the global norm, the clip and Adam's moments are fp32 (the kernels of the fp32 trainer).  After every optimiser step
 * the masters are rounded again into the bf16 images the encoder handle reads (lg_conv_tile_weights_bf16's layout, bit for bit), so the same
 * estimator predicts with the trained weights, and a fresh bf16 estimator built from the trainer's parameters gives its bits.  Deltas with a map's
 * shape (w.r.t. the pre-activations of conv 1-4) are stored as bf16, each rounded once when written from an fp32 accumulator times the fp32
 * derivative; row-shaped deltas stay fp32.  The two linear layers of the encoder keep the fp32 backward kernels, on exact fp32 expansions of the saved
 * bf16 rows and on fp32 transposed images that hold R(W).
 *
 * Workspace: the four saved maps and the two ping-pong delta buffers take 2 bytes per element instead of 4.
 *
 * Same library and conventions as lgestimator_train.h: device pointers unless marked HOST, 0 / negative status, ONE error channel: every refusal
 * leaves "<entry point>: <reason>" in the thread's message (lg_mlp_last_error of lgpolicy.h) and launches nothing.  No atomics: equal inputs give
 * equal bits. */
#ifndef LGESTIMATOR_TRAIN_BF16_H
#define LGESTIMATOR_TRAIN_BF16_H
#include <stdint.h>
#include "lgpolicy.h"
#include "lgestimator_train.h"
#ifdef __cplusplus
extern "C" {
#endif

/* One backward stage of the encoder, for lg_estimator_bf16train_backward_stage. */
enum lg_estimator_bf16_stage {
  LG_EST16_POOL_BACKWARD = 0,        /* delta_in (rows, 1024) w.r.t. the pooled rows -> delta_out: conv 4's map (rows, y, x, 64) */
  LG_EST16_DGRAD_CONV4 = 1,          /* delta_in: conv 4's map -> delta_out: conv 3's map */
  LG_EST16_DGRAD_CONV3 = 2,
  LG_EST16_DGRAD_CONV2 = 3,          /* delta_in: conv 2's map -> delta_out: conv 1's map */
  LG_EST16_WGRAD_CONV4 = 4,          /* delta_in: conv 4's map -> wgrad_out: dW (64, 128, 3, 3) then db (64), torch's layout */
  LG_EST16_WGRAD_CONV3 = 5,
  LG_EST16_WGRAD_CONV2 = 6,
  LG_EST16_WGRAD_CONV1 = 7,          /* reads the depth images the last group call was given: they must still stand */
  LG_EST16_LINEAR2 = 8,              /* depth_encoder.12: delta_in (rows, out_dim) -> delta_out (rows, 128) and wgrad_out: dW (out_dim, 128), db */
  LG_EST16_LINEAR1 = 9               /* depth_encoder.10: delta_in (rows, 128) -> delta_out (rows, 1024) (no activation below: the pooled rows) and dW (128, 1024), db */
};

/* lg_estimator_train_create for an encoder that IS LG_PREC_BF16 (lg_conv_encoder_create_precision); an fp32 encoder is refused by name, as
 * lg_estimator_train_create keeps refusing a bf16 one.  The other refusals are those of lg_estimator_train_create.  Destroyed by
 * lg_estimator_train_destroy. */
lg_estimator_train* lg_estimator_bf16train_create(lg_conv_encoder* encoder, lg_mlp* combine, lg_rnn* memory, lg_mlp* decoder, const lg_estimator_train_params* params,
                                                  double learning_rate, int64_t max_rows);

/* Rows (env, output pixel) per slab of the bf16 convolutions' weight-gradient pass. */
int32_t lg_estimator_bf16train_wgrad_slab_rows(void);

/* Stage k = 1..6 (conv 1-4, pool + flatten, linear 1) of the last group call's saved forward rows, expanded exactly to fp32 into `out` (device,
 * capacity floats): maps as (row, y, x, channel).  Refused: a NULL or fp32 trainer, k outside 1..6, no group call yet, capacity too small. */
int lg_estimator_bf16train_saved_stage(lg_estimator_train* trainer, int32_t k, float* out, int64_t capacity, void* stream);

/* One backward stage with the production kernels and grids, on the last group call's saved rows and the caller's delta: delta_in (device, fp32, the
 * last group's `rows` rows; the entry rounds it to bf16 where the stage reads bf16).  delta_out (device, fp32; the stage's output delta expanded
 * exactly where it is stored as bf16) and wgrad_out (device, fp32: the reduced dW then db in torch's layout) may be NULL where the stage has none or
 * the caller does not want it.  Overwrites the trainer's delta workspaces and the last group's gradient of that tensor.  Refused: a NULL or fp32
 * trainer, an unknown stage, NULL delta_in, rows that are not the last group's. */
int lg_estimator_bf16train_backward_stage(lg_estimator_train* trainer, int32_t stage, const float* delta_in, int64_t rows, float* delta_out, float* wgrad_out,
                                          void* stream);

#ifdef __cplusplus
}
#endif
#endif
