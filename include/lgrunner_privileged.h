/* lgrunner_privileged.h — C ABI of the on-policy runner's collection with PRIVILEGED CRITIC OBSERVATIONS (vendored rsl_rl:
 * runners/on_policy_runner.py:161-215, 278-286, 395-455: `alg.act(obs, privileged_obs)`, two normalisers): the critic reads the env's own row,
 * the actor a different one -- an observation history over the env's proprioceptive columns (legged_gym's AnymalStudent), or a column prefix.
 * Same library, conventions and error channel as lgrunner.h (lg_mlp_last_error); device pointers, asynchronous on the caller's stream.
 * Equal inputs give equal bits: no floating-point atomics, no workgroup waits on another. */
#ifndef LGRUNNER_PRIVILEGED_H
#define LGRUNNER_PRIVILEGED_H
#include <stdint.h>
#include "lgpolicy.h"
#include "lgrunner.h"
#ifdef __cplusplus
extern "C" {
#endif

/* lg_obsnorm_step on two handles over the same n rows: h_a on x_a -> out_a (rows stride_a floats apart, stride_a >= O_a), h_c on x_c -> out_c.
 * State, outputs and the handles' carried rows are bit for bit what the two single calls give: the same row slabs, the same fixed-order Chan
 * merge, the same rounding points.  Each of the three phases (float64 slab partials; merge and running update; apply) is ONE launch whose
 * grid's z index selects the handle, so a step costs three launches instead of six.  The widths may differ, and so may `until` and `count`:
 * each handle's freeze test (until >= 0 && count >= until) is its own; a phase only one handle needs runs as that handle's single launch.
 * out_a / out_c: may be x (in place) or NULL (that handle's update alone).  n = 0: nothing happens, LG_OK.
 * Refused as by the single call -- NULL handle, NULL rows, a stride smaller than the width, more than 65535 * 16 rows -- and for one handle
 * given twice or handles on different devices. */
int lg_obsnorm_step_pair(lg_obsnorm* h_a, const float* x_a, int64_t stride_a, float* out_a, lg_obsnorm* h_c, const float* x_c, int64_t stride_c,
                         float* out_c, int64_t n, int32_t update, void* stream);

/* What lg_runner_collect_privileged takes beyond lg_runner_collect.  O_c = the env's observation width = the input width of the critic (of
 * mem_c); O_a = the input width of the actor (of mem_a). */
typedef struct lg_runner_privileged {
  const lg_obs_history* history;     /* the actor's layer (lgpolicy.h), O_a = H * W; NULL: the actor reads the first O_a columns of the env's row */
  lg_obsnorm* critic_normalizer;     /* O_c wide; may be NULL.  hooks->normalizer is the ACTOR's here (O_a wide; may be NULL) */
  float* privileged_observations;    /* (T, n, O_c): the critic's rows */
  float* last_observations;          /* (n, O_a) or NULL: the actor's row after the last step, un-normalised */
} lg_runner_privileged;

/* lg_runner_collect with two observation streams; rows->observations is (T, n, O_a).  Per step t, without returning to the host:
 *   act     lg_policy_act / lg_policy_act_recurrent on observations[t] (actor) and privileged_observations[t] (critic), Philox call first_call + t;
 *   step    lg_step_transition: the next critic row straight into privileged_observations[t + 1] (after the last step into the critic
 *           normaliser's carried row); the time-out bootstrap uses values[t], the critic's value on the privileged row;
 *   actor   the actor's next row: lg_obs_history_step on `history` from the env's own RAW row (never the stored critic row, which is normalised in
 *           place), dones[t], noise call first_call + t or inject_u[t]; history NULL: a strided copy of the first O_a columns;
 *   norm    both new rows pass their normalisers in place (update = hooks->training): lg_obsnorm_step_pair with two handles, lg_obsnorm_step
 *           with one; the row after the last step of a stream becomes that handle's carried row;
 *   hooks   raw_rewards[t], extras[t], the memory resets on dones[t], as lg_runner_collect.
 * Row 0 of a stream is its handle's carried row when it holds one of n rows; else clamp(history, +-clip) (history NULL: the column prefix) for the
 * actor and the env's raw row for the critic, neither normalised nor counted.  last_values = the critic on the critic's last row (a recurrent
 * critic's memory advances once more), then lg_compute_returns, then the episode kernel.
 * Refused, with nothing launched: priv NULL or privileged_observations NULL; O_a that is not H * W of the history; without a history, O_a > O_c; a
 * normaliser whose width is not its stream's; one handle for both streams; and everything lg_runner_collect refuses. */
int lg_runner_collect_privileged(struct lg_ctx* env, lg_rnn* mem_a, lg_mlp* actor, lg_rnn* mem_c, lg_mlp* critic, const float* std, uint64_t seed,
                                 uint64_t first_call, int32_t T, float gamma, float lam, int32_t normalize_advantage, const lg_rollout* out,
                                 const lg_rollout_hidden* hid, float* h_a, float* c_a, float* h_c, float* c_c, const lg_runner_hooks* hooks,
                                 const lg_runner_privileged* priv, void* stream);

#ifdef __cplusplus
}
#endif
#endif
