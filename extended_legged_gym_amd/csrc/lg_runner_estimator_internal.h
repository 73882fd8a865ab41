// lg_runner_estimator_internal.h — what lg_sensors.hip (the estimation collection loop) and lg_runner_estimator.hip (the driver's entry point and the
// error kernel) share: the loop itself, behind the POLICY_ENTRY of lg_collect_estimation and of lg_runner_collect_estimation, and the two launches of
// the error figures the loop makes per step.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "lg_policy_internal.h"
#include "../../include/lgrunner_estimator.h"

// The one estimation collection loop (lg_sensors.hip).  driver: actions, or actor with an optional memory (and its state) and an optional normaliser;
// the four refusal members of the public struct are not read here.  stats NULL: no error figures.  A driver of {actions} or {actor} with stats NULL
// makes the launches lg_collect_estimation has always made.
int lg_estimation_collect(lg_sensor_rig* rig, const lg_estimation_driver* driver, int32_t T, const lg_estimation_out* out, const lg_estimation_nets* est,
                          const lg_estimation_stats* stats, void* stream);

// The checks of an lg_estimation_stats for n rows of R rays, and one step's two launches on pred / tgt (n, R): mse / mae written to the two
// pointers, the four rows written (first != 0) or updated (lg_runner_estimator.hip).
int lg_estimation_stats_ok(const lg_estimation_stats* stats, int64_t n, int32_t R);
int lg_estimation_errors_launch(const float* pred, const float* tgt, int64_t n, int32_t R, const lg_estimation_stats* stats, float* mse, float* mae, int first,
                                hipStream_t st);
