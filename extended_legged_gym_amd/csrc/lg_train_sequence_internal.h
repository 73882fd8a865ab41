// lg_train_sequence_internal.h -- the supervised sequence update the three sequence trainers share (lg_distill_train.hip, lg_distill_train_recurrent.hip,
// lg_estimator_train.hip): E * T steps cut into groups of G, each group one batch, a per-step mean loss of out - target with its seed gradient, the step
// means finished into a float64 sum, the remainder forward only, three or four doubles of stats.  The kernels and the host bodies live in
// lg_train_sequence.hip only; the checkpoint entry points are lg_train.hip's train_api_*.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <functional>
#include "lg_train_internal.h"
#include "lg_train_recurrent_internal.h"

#define SEQ_MAX_STEPS 65535          // steps of one batch: blockIdx.y of the loss kernel
enum { SEQ_LOSS_MSE = 0, SEQ_LOSS_HUBER = 1, SEQ_LOSS_L1 = 2 };          // lg_distill_loss and lg_estimator_loss, value for value (huber: delta 1)

struct SeqScalars {
  double acc;                        // sum of the step losses since the last clear
  int64_t steps;                     // steps in that sum
  int64_t optimizer_steps;           // optimiser steps since the last clear
};

// last_steps, last_update_steps, group_loss (max_rows) and seq_loss (seq_cap) are the core's
struct SeqCore : TrainCore {
  int out_w = 0;                     // columns of an output row: actions, or raycast outputs
  int64_t seq_cap = 0;
  int64_t* rows = nullptr;           // (max_rows) the group's row index; NULL: the trainer gathers no rows
  float* loss_part = nullptr;        // [step][block]
  float* step_tmp = nullptr;         // (max_rows) the means of the steps in flight
  SeqScalars* ss = nullptr;
};

// everything above and the core's two loss vectors, for groups of up to max_rows rows of out_w columns; false + message on failure
bool seq_alloc(SeqCore* c, int64_t max_rows, int out_w, bool want_rows);
// rows[j] = ((t0 + j / N) % T) * N + j % N for j < n: a group that wraps the epoch boundary is still one gathered batch
void seq_launch_rows(int64_t* rows, int64_t n, int64_t N, int64_t T, int64_t t0, hipStream_t st);
// out (nsteps, N * out_w) against target[(t0 + s) % T]: delta (may be NULL: forward only) gets dl / dout of the SUM of the steps' means; the step means
// go to group_loss and to seq_loss (either may be NULL: not written); train != 0 counts an optimiser step.
void seq_launch_loss(SeqCore* c, const float* out, const float* tgt, int64_t N, int64_t T, int64_t t0, int64_t nsteps, int loss_type, float* delta, float* group_loss,
                     float* seq_loss, int train, hipStream_t st);
// h, c (layers, layer_stride) (c may be NULL): rows j < N of every layer with dones[j] != 0 -> 0
void seq_launch_mask_rows(float* h, float* c, const float* dones, int64_t N, int H, int64_t layer_stride, int layers, hipStream_t st);

// The bodies of <prefix>_group's refusals, of <prefix>_update and of <prefix>_forward_outputs; the trainer's own check of the call runs first, in the
// exported function.  run_steps(first, nsteps, train, seq_loss, stream): the trainer's steps [first, first + nsteps) as one batch.  mem (may be NULL):
// the memory whose running state becomes the carry at the update's end.  stats (device, may be NULL): {mean loss, optimiser steps, gradient norm} and,
// with extra_norm (device), a fourth double from it.
typedef std::function<int(int64_t first, int64_t nsteps, bool train, float* seq_loss, hipStream_t st)> SeqSteps;
int seq_check_group(const SeqCore* c, int64_t N, int64_t first_step, int64_t num_steps);
int seq_update(SeqCore* c, int64_t T, int64_t N, int32_t E, int32_t G, const SeqSteps& run_steps, TrainMem* mem, void* stats, const float* extra_norm, void* stream);
int seq_forward_outputs(SeqCore* c, float* out, void* stream);
