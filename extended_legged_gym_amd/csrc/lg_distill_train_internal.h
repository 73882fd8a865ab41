// lg_distill_train_internal.h -- the behaviour-loss kernels of lg_distill_train.hip (the group's row index, the element losses with their seed
// gradient, the per-step means and the update's sums) as host launch functions: the recurrent student's trainer (lg_distill_train_recurrent.hip)
// runs its MLP stage through them.  The kernels live in lg_distill_train.hip only; both trainers' checkpoint entry points are lg_train.hip's train_api_*.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct DistillScalars {
  double acc;                        // sum of the step losses since the last clear
  int64_t steps;                     // steps in that sum
  int64_t optimizer_steps;           // optimiser steps since the last clear
};

// floats of loss_part for groups of up to max_rows rows of A actions
size_t distill_loss_floats(int64_t max_rows, int A);
// rows[j] = ((t0 + j / N) % T) * N + j % N for j < n
void distill_launch_rows(int64_t* rows, int64_t n, int64_t N, int64_t T, int64_t t0, hipStream_t st);
// out (nsteps, N * A) against target[(t0 + s) % T]: delta (may be NULL: forward only) gets dl / dout of the SUM of the steps' means; the step means go
// to step_tmp, to group_loss (train != 0 only) and to seq_loss (may be NULL); ds gets the sums.
void distill_launch_loss(const float* out, const float* tgt, int64_t N, int A, int64_t T, int64_t t0, int64_t nsteps, int loss_type, float* delta, float* loss_part,
                         float* step_tmp, float* group_loss, float* seq_loss, DistillScalars* ds, int train, hipStream_t st);
