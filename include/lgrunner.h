/* lgrunner.h — C ABI of the two device pieces the on-policy runner adds to the collection loop of lgpolicy.h (vendored rsl_rl:
 * runners/on_policy_runner.py:395-455): the running observation normaliser (modules/normalizer.py:14-76, `empirical_normalization`) and the
 * runner's episode bookkeeping (:508-525).  Same library, same conventions and the same error channel as lgpolicy.h (lg_mlp_last_error).
 * Device pointers unless marked HOST; every launch is asynchronous on the caller's hipStream_t.
 * Equal inputs give equal bits: no floating-point atomics, no workgroup waits on another; every sum and every merge has a fixed order. */
#ifndef LGRUNNER_H
#define LGRUNNER_H
#include <stdint.h>
#include "lgpolicy.h"
#ifdef __cplusplus
extern "C" {
#endif

/* One EmpiricalNormalization(shape=[O], eps, until).  On the device: _mean, _var, _std (O f32 each; 0, 1, 1), count (int64; 0) and the
 * CARRIED ROW, (n, O) f32 with a valid flag: the normalised observation after the last step of a collection, which is row 0 of the next one. */
typedef struct lg_obsnorm lg_obsnorm;

/* until < 0: None (the statistics never freeze).  NULL + a message for O < 1, eps that is not finite or < 0, a bad device. */
lg_obsnorm* lg_obsnorm_create(int32_t O, float eps, int64_t until, int device_id);
void lg_obsnorm_destroy(lg_obsnorm* h);

/* HOST copies of _mean, _var, _std (O f32 each) and count, unchanged bits either way; each pointer may be NULL.  Both wait for `stream`. */
int lg_obsnorm_get_state(lg_obsnorm* h, float* mean_host, float* var_host, float* std_host, int64_t* count_host, void* stream);
int lg_obsnorm_set_state(lg_obsnorm* h, const float* mean_host, const float* var_host, const float* std_host, int64_t count, void* stream);

/* The module's forward on x (n rows of O, row_stride floats apart, row_stride >= O).  update != 0 and not (until >= 0 and count >= until):
 *     count += n;  rate = n / count;  mean_x, var_x = the column mean and BIASED variance of the n rows;  delta = mean_x - mean;
 *     mean += rate * delta;  var += rate * (var_x - var + delta * (mean_x - mean_new));  std = sqrt(var)
 * then, always, out = (x - mean) / (std + eps) with the statistics AFTER the update.  out has x's row stride and may be x (in place);
 * out NULL: the update alone (the module's update()).  n = 0: nothing happens, LG_OK.
 * Three launches: per-workgroup (count, mean, M2) partials of the columns in float64; their pairwise (Chan) merge in a fixed order and the
 * running update (float64 arithmetic on the f32 state, rounded once); the normalisation (f32, the module's two operations).
 * At most 65535 * 16 rows per call. */
int lg_obsnorm_step(lg_obsnorm* h, const float* x, int64_t n, int64_t row_stride, int32_t update, float* out, void* stream);

/* out = y * (std + eps) + mean (the module's inverse); strides and aliasing as lg_obsnorm_step. */
int lg_obsnorm_inverse(lg_obsnorm* h, const float* y, int64_t n, int64_t row_stride, float* out, void* stream);

/* The carried row: returns 1 and copies it to `out` ((n, O) contiguous; may be NULL: report only) when one of n rows is held, 0 when none is
 * (or it has another n), negative on error.  forget invalidates it: the next collection starts from the env's raw observation again. */
int lg_obsnorm_carried(lg_obsnorm* h, float* out, int64_t n, void* stream);
int lg_obsnorm_forget_carried(lg_obsnorm* h);

/* The runner's episode bookkeeping over one collection.  All device memory, f32. */
typedef struct lg_runner_episode {
  float* raw_rewards;          /* (T, n): the env's rew_buf after each step, WITHOUT the time-out bootstrap lg_rollout.rewards carries */
  float* extras;               /* (T, K): the env's whole extras_episode tensor after each step (K = its length): infos["episode"] of that step */
  float* cur_reward_sum;       /* (n): the live sums, updated in place */
  float* cur_episode_length;   /* (n) */
  float* ep_return;            /* (T, n): the finished episode's sum where dones[t] > 0, else 0 */
  float* ep_length;            /* (T, n) */
} lg_runner_episode;

typedef struct lg_runner_hooks {
  lg_obsnorm* normalizer;      /* may be NULL */
  int32_t training;            /* the normaliser's mode: != 0 updates the statistics on every new row */
  lg_runner_episode* episode;  /* may be NULL */
} lg_runner_hooks;

/* lg_collect_rollout (mem_a, mem_c, hid and the four state pointers NULL) / lg_collect_rollout_recurrent with the two hooks; hooks NULL or
 * both members NULL: the same rows, bit for bit.
 * normalizer: row 0 is the handle's carried row when it holds one of n rows, else the env's raw observation, neither normalised nor counted
 * (the first observation of learn(), on_policy_runner.py:364-365, never passes the normaliser).  After every step the new raw row is
 * normalised in place by lg_obsnorm_step(update = training) -- the row after the last step too, which becomes the carried row: T steps, T
 * updates.  last_values is evaluated on the carried row.  The env's own obs_buf stays raw.  One handle serves actor and critic here; a critic
 * with privileged observations of its own, and a normaliser of its own, is lgrunner_privileged.h (lg_runner_collect_privileged).
 * episode: raw_rewards[t] and extras[t] are copied after step t; after the loop one kernel, one thread per env, walks the T steps:
 * sum += r; len += 1; if dones[t] > 0: emit and zero.  The host takes dones.nonzero() once: its (t, env) order is the reference's. */
int lg_runner_collect(struct lg_ctx* env, lg_rnn* mem_a, lg_mlp* actor, lg_rnn* mem_c, lg_mlp* critic, const float* std, uint64_t seed,
                      uint64_t first_call, int32_t T, float gamma, float lam, int32_t normalize_advantage, const lg_rollout* out,
                      const lg_rollout_hidden* hid, float* h_a, float* c_a, float* h_c, float* c_c, const lg_runner_hooks* hooks, void* stream);

/* The episode kernel alone over given (T, n) rows. */
int lg_runner_episode_track(const float* rewards, const float* dones, int32_t T, int64_t n, float* cur_reward_sum, float* cur_episode_length,
                            float* ep_return, float* ep_length, void* stream);

#ifdef __cplusplus
}
#endif
#endif
