/* lgrunner_distill.h — C ABI of the on-policy runner's collection for DISTILLATION (vendored rsl_rl: runners/on_policy_runner.py:395-431 with
 * algorithms/distillation.py:89-105: `alg.act(obs, privileged_obs)`, `process_env_step`, two normalisers, the episode bookkeeping): the teacher
 * reads the env's own row, the student an observation history over the env's proprioceptive columns (legged_gym's AnymalStudent) or a column prefix.
 * Same library, conventions and error channel as lgrunner.h (lg_mlp_last_error); device pointers, asynchronous on the caller's stream.
 * This unit holds no kernel: it strings lg_distill_act*, lg_step_transition, lg_obs_history_step, lg_obsnorm_step(_pair) and
 * lg_runner_episode_track together, each of which gives equal bits for equal inputs. */
#ifndef LGRUNNER_DISTILL_H
#define LGRUNNER_DISTILL_H
#include <stdint.h>
#include "lgpolicy.h"
#include "lgrunner.h"
#ifdef __cplusplus
extern "C" {
#endif

/* What the two calls below take beyond lg_collect_distillation(_recurrent).  O_t = the env's observation width = the input width of the teacher (of
 * mem_t); O_s = the input width of the student (of mem_s). */
typedef struct lg_runner_distill {
  lg_obsnorm* student_normalizer;   /* O_s wide; may be NULL */
  lg_obsnorm* teacher_normalizer;   /* O_t wide (the env's row); may be NULL */
  int32_t training;                 /* both handles' mode: update the running statistics or only apply */
  const lg_runner_episode* episode; /* lgrunner.h; may be NULL */
} lg_runner_distill;

/* lg_collect_distillation with the runner's hooks; hooks NULL or all members NULL: the same rows, bit for bit.  Per step t, without returning
 * to the host:
 *   act      lg_distill_act on observations[t] (student) and privileged_observations[t] (teacher), Philox call first_call + t;
 *   step     lg_step_transition: the next teacher row straight into privileged_observations[t + 1] (after the last step into the teacher
 *            normaliser's carried row); rewards[t] is the env's raw reward: no value row, no time-out bootstrap;
 *   student  the student's next row: lg_obs_history_step on `history` from the env's own RAW row (never the stored teacher row, which is normalised
 *            in place), dones[t], noise call first_call + t or inject_u[t]; history NULL: a strided copy of the first O_s columns.  After the last
 *            step the un-normalised row goes to rows->last_observations and its normalised copy to the student normaliser's carried row;
 *   norm     both new rows pass their normalisers (update = hooks->training; the reference keeps the teacher's in training mode too,
 *            on_policy_runner.py:736-738): lg_obsnorm_step_pair with two handles, lg_obsnorm_step with one;
 *   hooks    episode->raw_rewards[t] and episode->extras[t] are copied after the step.
 * Row 0 of a stream is its handle's carried row when it holds one of n rows; else clamp(history, +-clip) (history NULL: the column prefix) for the
 * student and the env's raw row for the teacher, neither normalised nor counted.  The episode kernel (lg_runner_episode_track) follows the loop on
 * the same stream over rows->rewards and rows->dones.  The carried rows are committed only when the call succeeds.
 * Refused, with nothing launched: everything lg_collect_distillation refuses; a normaliser whose width is not its stream's; one handle for both
 * streams; a handle on another device than the networks; an episode with a NULL row. */
int lg_runner_collect_distillation(struct lg_ctx* env, lg_mlp* student, lg_mlp* teacher, const float* std, uint64_t seed, uint64_t first_call, int32_t T,
                                   const lg_obs_history* history, const lg_distill_rollout* rows, const lg_runner_distill* hooks, void* stream);

/* The same with a memory in front of the student (and, mem_t set, of the teacher): lg_distill_act_recurrent per step, both memories reset on
 * dones[t] after the step; the state pointers are those of lg_collect_distillation_recurrent. */
int lg_runner_collect_distillation_recurrent(struct lg_ctx* env, lg_rnn* mem_s, lg_mlp* student, lg_rnn* mem_t, lg_mlp* teacher, const float* std, uint64_t seed,
                                             uint64_t first_call, int32_t T, const lg_obs_history* history, const lg_distill_rollout* rows, float* h_s0,
                                             float* c_s0, float* h_t0, float* c_t0, float* h_s, float* c_s, float* h_t, float* c_t,
                                             const lg_runner_distill* hooks, void* stream);

#ifdef __cplusplus
}
#endif
#endif
