/* lgrunner_estimator.h — C ABI of what the terrain-estimator runner adds to the estimation collection of lgsensors.h (vendored rsl_rl:
 * runners/terrain_estimator_runner.py): the collection loop of `learn` (:392-438) and the evaluation loop of `play` (:637-730) as ONE loop whose
 * robot is moved by a DRIVER -- pre-drawn actions, a feed-forward actor, the same actor behind an observation normaliser, or a recurrent policy --
 * and the error figures `play` prints per step (:666-670), with per-ray sums beside them, from one kernel.
 * Same library, conventions and error channel as lgpolicy.h / lgsensors.h (lg_mlp_last_error): every refusal leaves "<entry point>: <reason>" with
 * nothing launched and nothing stepped.  Device pointers unless marked HOST; every launch is asynchronous on the caller's hipStream_t.
 * Equal inputs give equal bits: no floating-point atomics, every sum has a fixed order. */
#ifndef LGRUNNER_ESTIMATOR_H
#define LGRUNNER_ESTIMATOR_H
#include <stdint.h>
#include "lgpolicy.h"
#include "lgrunner.h"
#include "lgsensors.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Who moves the robot during the collection: the `pretrained_policy` of the runner (terrain_estimator_runner.py:162-245, used at :402-427 and
 * :686-709), in the reference an ActorCritic / ActorCriticRecurrent behind an optional observation standardisation.  Exactly one of
 *   actions                  (T, n, A) pre-drawn rows (the 0.5 * randn of :427 drawn before the call), everything else NULL / 0;
 *   actor                    act_inference of an ActorCritic (modules/actor_critic.py:129-131) on the env's raw observation row: lg_mlp_forward,
 *                            a narrower actor reads the row's column prefix, a wide actor (lgpolicy_wide.h) the wide forward -- as
 *                            lg_collect_estimation;
 *   actor + normalizer       the same behind an lg_obsnorm in inference mode (lgrunner.h; the runner's `empirical_normalization`,
 *                            on_policy_runner.py:717-727): out = (x - mean) / (std + eps) by lg_obsnorm_step(update = 0) into a scratch row; the
 *                            env's own row stays raw, the moments and the count are not touched.  The handle is as wide as the policy's input;
 *   memory + actor           act_inference of an ActorCriticRecurrent (modules/actor_critic_recurrent.py:82-85): lg_rnn_step on the row (a
 *                            narrow memory or one of lg_rnn_create_wide), then lg_mlp_forward on the top layer's h' -- the launches of
 *                            lg_policy_act_recurrent for the mean, no sampling.  h / c: the policy memory's live state (L, n, H), in place; after
 *                            each step lg_rnn_reset_rows on the step's dones (Memory.reset, networks/memory.py:45-51), a launch of its own beside
 *                            the estimator memory's reset.  A normaliser may stand in front.
 * The four last members exist to be refused by name: the loop runs the deterministic actor of one observation stream and nothing else. */
typedef struct lg_estimation_driver {
  const float* actions;                   /* (T, n, A), or NULL */
  lg_mlp* actor;                          /* or NULL */
  lg_rnn* memory;                         /* memory_a, or NULL: feed-forward */
  float* h;                               /* (L, n, H) with a memory */
  float* c;                               /* an LSTM's cell state; NULL for a GRU */
  lg_obsnorm* normalizer;                 /* or NULL */
  int32_t normalizer_training;            /* != 0: refused (the statistics do not move during estimator training) */
  lg_mlp* critic;                         /* not NULL: refused (nothing here reads a value) */
  const float* std;                       /* not NULL: refused (sampling; `deterministic=False` of play, :703-704, is not built) */
  const float* privileged_observations;   /* not NULL: refused (a second observation stream) */
} lg_estimation_driver;

/* The figures of `play` (terrain_estimator_runner.py:666-670) for every step of a call, and what they do not show: which rays are wrong.
 * mse[t] = mean((p - t)^2), mae[t] = mean(|p - t|) over the step's (n, R) entries; the four rows of width R hold, summed over the T steps of the
 * call and all envs (written, not added to, by the call's first step): sum of squared error, sum of absolute error, sum of signed error p - t, and
 * the largest absolute error.  workspace: lg_estimation_errors_workspace(n, R) floats the kernel's partial sums pass through. */
typedef struct lg_estimation_stats {
  float* mse;                 /* (T) */
  float* mae;                 /* (T) */
  float* ray_sq_error;        /* (R) */
  float* ray_abs_error;       /* (R) */
  float* ray_bias;            /* (R) */
  float* ray_max_error;       /* (R) */
  float* workspace;
  int64_t workspace_floats;
} lg_estimation_stats;

/* The floats of `workspace` for n rows of R rays: 4 R per row slab, at most 128 slabs.  Negative for n < 1 or R outside 1..65536.  No device work. */
int64_t lg_estimation_errors_workspace(int64_t n, int32_t R);

/* The error figures alone, over `steps` steps of predictions / targets (steps, n, R): what the loop below launches per step, through the same code.
 * Two launches per step.  estimation_error_kernel: a capped grid of (row slab, tile of 64 column units) workgroups; a lane owns a column unit
 * -- four adjacent rays read with one 16-byte load where R % 4 == 0 and both pointers are 16-byte aligned, one ray otherwise -- and walks its
 * slab's rows with a grid-stride loop, four waves on every fourth row, merged through LDS in wave order into one partial per slab.  The finish,
 * one workgroup: per ray the slabs in ascending order (fp32), the rows updated in fp32; the two means from the rays' sums in ascending order per
 * thread and a fixed tree across threads, in float64, rounded once.  No atomics: two runs give equal bits.
 * Refused: a NULL pointer, steps < 1, n < 1, R outside 1..65536, a workspace smaller than lg_estimation_errors_workspace(n, R). */
int lg_estimation_errors(const float* predictions, const float* targets, int32_t steps, int64_t n, int32_t R, const lg_estimation_stats* stats,
                         void* stream);

/* lg_collect_estimation (lgsensors.h) with a driver in the place of the bare actor and, optionally, the error figures: the collection loop of
 * TerrainEstimatorRunner.learn (terrain_estimator_runner.py:392-438) and, with `nets` and `stats`, the loop of play (:661-720) without storage
 * of its own -- the SAME loop body as lg_collect_estimation (one function, csrc/lg_sensors.hip).  Per step t:
 *   rows, estimator          as lg_collect_estimation;
 *   errors                   (stats and nets both given) the two launches of lg_estimation_errors on predictions[t] / raycast_targets[t];
 *   actions                  the driver's (above);
 *   step, estimator reset    as lg_collect_estimation;
 *   policy reset             (a recurrent driver) lg_rnn_reset_rows on the policy's memory.
 * With a raw-row actor or pre-drawn actions and stats NULL the launches are lg_collect_estimation's, one for one.
 * Refused: everything lg_collect_estimation refuses; a NULL driver; a critic; sampling (std); a normaliser in training mode; two observation
 * streams; a memory without an actor or without its state; an actor that does not read the memory's hidden row; a normaliser of another width
 * than the policy's input or on another device; stats without nets, or with a NULL member or a short workspace. */
int lg_runner_collect_estimation(lg_sensor_rig* rig, const lg_estimation_driver* driver, int32_t T, const lg_estimation_out* out,
                                 const lg_estimation_nets* nets, const lg_estimation_stats* stats, void* stream);

#ifdef __cplusplus
}
#endif
#endif
