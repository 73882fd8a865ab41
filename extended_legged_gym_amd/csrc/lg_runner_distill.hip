// lg_runner_distill.hip — the runner's collection for distillation (include/lgrunner_distill.h): the two entry points that hand the runner's hooks
// (two normalisers, the episode rows) to the one distillation loop (lg_policy.hip, lg_policy_collect_distillation) and run the episode kernel
// (lg_runner.hip) behind it.  No kernel lives here: every launch is one the plain collectors, the normaliser and the tracker already make.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>

#include "lg_device.h"
#include "lg_policy_internal.h"
#include "lg_runner_internal.h"
#include "../../include/lgpolicy.h"
#include "../../include/lgrunner.h"
#include "../../include/lgrunner_distill.h"
#include "../../include/lgstep.h"

// the body of both entry points, behind their POLICY_ENTRY
static int runner_collect_distillation(lg_ctx* env, int recurrent, lg_rnn* mem_s, lg_mlp* student, lg_rnn* mem_t, lg_mlp* teacher, const float* std, uint64_t seed,
                                       uint64_t first_call, int32_t T, const lg_obs_history* history, const lg_distill_rollout* rows, float* h_s0, float* c_s0,
                                       float* h_t0, float* c_t0, float* h_s, float* c_s, float* h_t, float* c_t, const lg_runner_distill* hooks, void* stream) {
  DistillHooks dh;
  const lg_runner_episode* ep = hooks ? hooks->episode : nullptr;
  if (hooks) {
    dh.normalizer_s = hooks->student_normalizer; dh.normalizer_t = hooks->teacher_normalizer; dh.update = hooks->training != 0;
    for (const lg_obsnorm* h : {hooks->student_normalizer, hooks->teacher_normalizer})
      if (h && student && h->device != student->device) return lg_policy_fail(LG_ERR_INVALID, "a normaliser is on another device than the networks");
  }
  if (ep) {
    if (!ep->raw_rewards || !ep->extras || !ep->cur_reward_sum || !ep->cur_episode_length || !ep->ep_return || !ep->ep_length)
      return lg_policy_fail(LG_ERR_INVALID, "null episode row");
    dh.raw_rewards = ep->raw_rewards; dh.extras = ep->extras;
  }
  int rc = lg_policy_collect_distillation(env, recurrent, mem_s, student, mem_t, teacher, std, seed, first_call, T, history, rows, h_s0, c_s0, h_t0, c_t0, h_s, c_s,
                                          h_t, c_t, &dh, stream);
  if (rc != LG_OK || !ep) return rc;
  EnvRewardRows env_rows;
  if ((rc = lg_policy_reward_rows(env, &env_rows)) != LG_OK) return rc;
  return lg_runner_episode_track(rows->rewards, rows->dones, T, env_rows.n, ep->cur_reward_sum, ep->cur_episode_length, ep->ep_return, ep->ep_length, stream);
}

extern "C" {

int lg_runner_collect_distillation(lg_ctx* env, lg_mlp* student, lg_mlp* teacher, const float* std, uint64_t seed, uint64_t first_call, int32_t T,
                                   const lg_obs_history* history, const lg_distill_rollout* rows, const lg_runner_distill* hooks, void* stream) {
  POLICY_ENTRY;
  return runner_collect_distillation(env, 0, nullptr, student, nullptr, teacher, std, seed, first_call, T, history, rows, nullptr, nullptr, nullptr, nullptr, nullptr,
                                     nullptr, nullptr, nullptr, hooks, stream);
}

int lg_runner_collect_distillation_recurrent(lg_ctx* env, lg_rnn* mem_s, lg_mlp* student, lg_rnn* mem_t, lg_mlp* teacher, const float* std, uint64_t seed,
                                             uint64_t first_call, int32_t T, const lg_obs_history* history, const lg_distill_rollout* rows, float* h_s0,
                                             float* c_s0, float* h_t0, float* c_t0, float* h_s, float* c_s, float* h_t, float* c_t,
                                             const lg_runner_distill* hooks, void* stream) {
  POLICY_ENTRY;
  return runner_collect_distillation(env, 1, mem_s, student, mem_t, teacher, std, seed, first_call, T, history, rows, h_s0, c_s0, h_t0, c_t0, h_s, c_s, h_t, c_t,
                                     hooks, stream);
}

}  // extern "C"
