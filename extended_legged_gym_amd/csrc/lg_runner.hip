// lg_runner.hip — gfx950 kernels of the on-policy runner's two device pieces (include/lgrunner.h): the running observation normaliser
// (rsl_rl modules/normalizer.py:14-76) and the episode bookkeeping (runners/on_policy_runner.py:508-525), and the collector that runs them
// between the launches of the one-call collection loop (lg_policy.hip).
//
// Column moments of an (n, O) batch, 4096 x 235 in the flagship (3.8 MB: latency-bound, a few microseconds of memory time).  A workgroup is four
// waves; a wave's 64 lanes are 64 adjacent columns (one 256-byte row segment per load), the four waves take every fourth row of the workgroup's
// row slab.  The grid is (row slabs <= 128, column tiles of 64): 512 workgroups at 4096 x 235, two per compute unit, 8 rows per lane, all eight
// loads in flight before the first is used.  A lane sums x - x0 and its square in float64, x0 its own first value (one pass; in float64 the
// shifted sums lose nothing a float32 result can see): (count, mean, M2).  The four waves' triples meet in LDS and wave 0 merges them with the
// pairwise rule of Chan et al. in wave order; a second, tiny launch merges the slabs' triples -- sixteen runs of slabs side by side, each in slab
// order, then the sixteen pairwise -- and applies the running update; a third normalises.  No atomics, no workgroup waits on another.
#include <hip/hip_runtime.h>
#include <cmath>
#include <math.h>
#include <stdint.h>
#include <string>
#include <vector>

#include "lg_device.h"
#include "lg_policy_internal.h"
#include "../../include/lgpolicy.h"
#include "../../include/lgrunner.h"
#include "../../include/lgstep.h"
#include "lg_runner_internal.h"          // the handle and the bodies of the three normaliser kernels, shared with lg_runner_privileged.hip

__global__ __launch_bounds__(ON_COLS * ON_WAVES) void obsnorm_partial_kernel(const float* __restrict__ x, int64_t n, int64_t stride, int O, int64_t slab_rows,
                                                                             double* __restrict__ partial) {
  __shared__ double sh[3][ON_WAVES][ON_COLS];
  obsnorm_partial_body(sh, blockIdx.x, blockIdx.y, x, n, stride, O, slab_rows, partial);
}

__global__ __launch_bounds__(ON_COLS * ON_UPD_WAVES) void obsnorm_update_kernel(const double* __restrict__ partial, int slabs, int O, double rate, float* mean,
                                                                                float* var, float* sd, int64_t* count, int64_t new_count) {
  __shared__ double sh[3][ON_UPD_WAVES][ON_COLS];
  obsnorm_update_body(sh, blockIdx.x, partial, slabs, O, rate, mean, var, sd, count, new_count);
}

__global__ __launch_bounds__(ON_COLS * ON_WAVES) void obsnorm_apply_kernel(const float* x, int64_t n, int64_t stride, int O, const float* __restrict__ mean,
                                                                           const float* __restrict__ sd, float eps, int inverse, float* out) {
  obsnorm_apply_body(blockIdx.x, blockIdx.y, x, n, stride, O, mean, sd, eps, inverse, out);
}

// one thread per env walks the T steps: on_policy_runner.py:516-525
__global__ __launch_bounds__(256) void runner_episode_kernel(const float* __restrict__ rewards, const float* __restrict__ dones, int T, int64_t n, float* cur_sum,
                                                             float* cur_len, float* __restrict__ ep_return, float* __restrict__ ep_length) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  float s = cur_sum[e], l = cur_len[e];
  for (int t = 0; t < T; ++t) {
    const int64_t i = (int64_t)t * n + e;
    s += rewards[i]; l += 1.f;
    const bool done = dones[i] > 0.f;
    ep_return[i] = done ? s : 0.f; ep_length[i] = done ? l : 0.f;
    if (done) { s = 0.f; l = 0.f; }
  }
  cur_sum[e] = s; cur_len[e] = l;
}

int obsnorm_rows_ok(const lg_obsnorm* h, const float* x, int64_t n, int64_t row_stride) {
  if (!h) return lg_policy_fail(LG_ERR_INVALID, "null normaliser");
  if (n < 0 || (n > 0 && (!x || row_stride < h->O))) return lg_policy_fail(LG_ERR_INVALID, "null rows, n < 0 or row_stride < O");
  if (n > 0 && (n > INT64_MAX / row_stride || n > (int64_t)65535 * ON_APPLY_ROWS)) return lg_policy_fail(LG_ERR_INVALID, "too many rows");
  return LG_OK;
}

static int obsnorm_apply(lg_obsnorm* h, const float* x, int64_t n, int64_t row_stride, int inverse, float* out, hipStream_t st) {
  hipLaunchKernelGGL(obsnorm_apply_kernel, dim3((h->O + ON_COLS - 1) / ON_COLS, (unsigned)((n + ON_APPLY_ROWS - 1) / ON_APPLY_ROWS)), dim3(ON_COLS * ON_WAVES), 0, st,
                     x, n, row_stride, h->O, h->state, h->state + 2 * (size_t)h->O, h->eps, inverse, out);
  POLICY_TRY(hipGetLastError());
  return LG_OK;
}

int lg_obsnorm_carried_begin(lg_obsnorm* h, int64_t n, int64_t O, float** row, bool* valid) {
  if (O != h->O) return lg_policy_fail(LG_ERR_INVALID, "the normaliser's width is not the env's observation width");
  DeviceScope ds_(h->device);
  if (h->carried_n != n) {
    if (h->carried) { POLICY_TRY(hipDeviceSynchronize()); POLICY_TRY(hipFree(h->carried)); h->carried = nullptr; }
    h->carried_n = 0; h->carried_valid = false;
    POLICY_TRY(hipMalloc((void**)&h->carried, (size_t)n * O * 4));
    h->carried_n = n;
  }
  *row = h->carried; *valid = h->carried_valid;
  h->carried_valid = false;
  return LG_OK;
}

void lg_obsnorm_carried_commit(lg_obsnorm* h) { h->carried_valid = true; }

extern "C" {

lg_obsnorm* lg_obsnorm_create(int32_t O, float eps, int64_t until, int device_id) {
  POLICY_ENTRY;
  if (O < 1 || O > (1 << 20) || !(eps >= 0.f) || !std::isfinite(eps)) { lg_policy_fail(LG_ERR_INVALID, "O out of range (1..2^20), or eps negative or not finite"); return nullptr; }
  if (!lg_policy_device_ok(device_id)) return nullptr;
  DeviceScope ds_(device_id);
  lg_obsnorm* h = new lg_obsnorm();
  h->O = O; h->eps = eps; h->until = until < 0 ? -1 : until; h->device = device_id;
  if (hipMalloc((void**)&h->state, (size_t)3 * O * 4) != hipSuccess || hipMalloc((void**)&h->count_dev, 8) != hipSuccess ||
      hipMalloc((void**)&h->partial, (size_t)ON_MAX_SLABS * 3 * O * 8) != hipSuccess) {
    lg_policy_fail(LG_ERR_HIP, "device allocation failed");
    lg_obsnorm_destroy(h);
    return nullptr;
  }
  std::vector<float> init((size_t)3 * O, 1.f);
  for (int i = 0; i < O; ++i) init[i] = 0.f;
  const int64_t zero = 0;
  if (hipMemcpy(h->state, init.data(), init.size() * 4, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(h->count_dev, &zero, 8, hipMemcpyHostToDevice) != hipSuccess) {
    lg_policy_fail(LG_ERR_HIP, "state upload failed");
    lg_obsnorm_destroy(h);
    return nullptr;
  }
  return h;
}

void lg_obsnorm_destroy(lg_obsnorm* h) {
  if (!h) return;
  DeviceScope ds_(h->device);
  (void)hipFree(h->state); (void)hipFree(h->count_dev); (void)hipFree(h->partial); (void)hipFree(h->carried);
  delete h;
}

int lg_obsnorm_get_state(lg_obsnorm* h, float* mean_host, float* var_host, float* std_host, int64_t* count_host, void* stream) {
  POLICY_ENTRY;
  if (!h) return lg_policy_fail(LG_ERR_INVALID, "null normaliser");
  DeviceScope ds_(h->device);
  POLICY_TRY(hipStreamSynchronize((hipStream_t)stream));
  float* dst[3] = {mean_host, var_host, std_host};
  for (int k = 0; k < 3; ++k)
    if (dst[k]) POLICY_TRY(hipMemcpy(dst[k], h->state + (size_t)k * h->O, (size_t)h->O * 4, hipMemcpyDeviceToHost));
  if (count_host) POLICY_TRY(hipMemcpy(count_host, h->count_dev, 8, hipMemcpyDeviceToHost));
  return LG_OK;
}

int lg_obsnorm_set_state(lg_obsnorm* h, const float* mean_host, const float* var_host, const float* std_host, int64_t count, void* stream) {
  POLICY_ENTRY;
  if (!h) return lg_policy_fail(LG_ERR_INVALID, "null normaliser");
  if (count < 0) return lg_policy_fail(LG_ERR_INVALID, "count < 0");
  DeviceScope ds_(h->device);
  POLICY_TRY(hipStreamSynchronize((hipStream_t)stream));
  const float* src[3] = {mean_host, var_host, std_host};
  for (int k = 0; k < 3; ++k)
    if (src[k]) POLICY_TRY(hipMemcpy(h->state + (size_t)k * h->O, src[k], (size_t)h->O * 4, hipMemcpyHostToDevice));
  POLICY_TRY(hipMemcpy(h->count_dev, &count, 8, hipMemcpyHostToDevice));
  h->count = count;
  return LG_OK;
}

int lg_obsnorm_step(lg_obsnorm* h, const float* x, int64_t n, int64_t row_stride, int32_t update, float* out, void* stream) {
  POLICY_ENTRY;
  const int rc = obsnorm_rows_ok(h, x, n, row_stride);
  if (rc != LG_OK) return rc;
  if (n == 0) return LG_OK;
  DeviceScope ds_(h->device);
  hipStream_t st = (hipStream_t)stream;
  if (update && !(h->until >= 0 && h->count >= h->until)) {
    int64_t slab_rows;
    const int slabs = obsnorm_slabs(n, &slab_rows);
    hipLaunchKernelGGL(obsnorm_partial_kernel, dim3(slabs, (h->O + ON_COLS - 1) / ON_COLS), dim3(ON_COLS * ON_WAVES), 0, st, x, n, row_stride, h->O, slab_rows,
                       h->partial);
    h->count += n;
    float* s = h->state;
    hipLaunchKernelGGL(obsnorm_update_kernel, dim3((h->O + ON_COLS - 1) / ON_COLS), dim3(ON_COLS * ON_UPD_WAVES), 0, st, (const double*)h->partial, slabs, h->O, (double)n / (double)h->count, s,
                       s + h->O, s + 2 * (size_t)h->O, h->count_dev, h->count);
    POLICY_TRY(hipGetLastError());
  }
  return out ? obsnorm_apply(h, x, n, row_stride, 0, out, st) : LG_OK;
}

int lg_obsnorm_inverse(lg_obsnorm* h, const float* y, int64_t n, int64_t row_stride, float* out, void* stream) {
  POLICY_ENTRY;
  const int rc = obsnorm_rows_ok(h, y, n, row_stride);
  if (rc != LG_OK) return rc;
  if (n > 0 && !out) return lg_policy_fail(LG_ERR_INVALID, "null output rows");
  if (n == 0) return LG_OK;
  DeviceScope ds_(h->device);
  return obsnorm_apply(h, y, n, row_stride, 1, out, (hipStream_t)stream);
}

int lg_obsnorm_carried(lg_obsnorm* h, float* out, int64_t n, void* stream) {
  POLICY_ENTRY;
  if (!h) return lg_policy_fail(LG_ERR_INVALID, "null normaliser");
  if (!h->carried_valid || h->carried_n != n) return 0;
  DeviceScope ds_(h->device);
  if (out) POLICY_TRY(hipMemcpyAsync(out, h->carried, (size_t)n * h->O * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return 1;
}

int lg_obsnorm_forget_carried(lg_obsnorm* h) {
  POLICY_ENTRY;
  if (!h) return lg_policy_fail(LG_ERR_INVALID, "null normaliser");
  h->carried_valid = false;
  return LG_OK;
}

int lg_runner_episode_track(const float* rewards, const float* dones, int32_t T, int64_t n, float* cur_reward_sum, float* cur_episode_length, float* ep_return,
                            float* ep_length, void* stream) {
  POLICY_ENTRY;
  if (!rewards || !dones || !cur_reward_sum || !cur_episode_length || !ep_return || !ep_length || T < 1 || n < 0)
    return lg_policy_fail(LG_ERR_INVALID, "null row, T < 1 or n < 0");
  if (n == 0) return LG_OK;
  const int dev = lg_policy_device_of(rewards);
  if (dev < 0) return lg_policy_fail(LG_ERR_INVALID, "rewards is not device memory");
  DeviceScope ds_(dev);
  hipLaunchKernelGGL(runner_episode_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rewards, dones, T, n, cur_reward_sum,
                     cur_episode_length, ep_return, ep_length);
  POLICY_TRY(hipGetLastError());
  return LG_OK;
}

}  // extern "C"

// lg_runner_collect (priv NULL) and lg_runner_collect_privileged: the runner's structs become the loop's hooks, the loop runs (lg_policy.hip), and the
// episode bookkeeping follows it on the same stream.  The message prefix is the caller's: each entry point opens its own POLICY_ENTRY.
int lg_runner_collect_both(lg_ctx* env, lg_rnn* mem_a, lg_mlp* actor, lg_rnn* mem_c, lg_mlp* critic, const float* std, uint64_t seed, uint64_t first_call, int32_t T,
                           float gamma, float lam, int32_t normalize_advantage, const lg_rollout* out, const lg_rollout_hidden* hid, float* h_a, float* c_a, float* h_c,
                           float* c_c, const lg_runner_hooks* hooks, const lg_runner_privileged* priv, lg_sensor_rig* sensors, void* stream) {
  if (!env || !actor || !critic || !std || !out || T <= 0) return lg_policy_fail(LG_ERR_INVALID, "null argument or T < 1");
  if ((mem_a != nullptr) != (mem_c != nullptr) || (mem_a && !hid)) return lg_policy_fail(LG_ERR_INVALID, "a recurrent policy needs both memories and the hidden-state rows");
  CollectHooks ch;
  ch.sensors = sensors;
  const lg_runner_episode* ep = hooks ? hooks->episode : nullptr;
  if (hooks) { ch.normalizer = hooks->normalizer; ch.update = hooks->training != 0; }
  if (priv) {
    ch.history = priv->history; ch.normalizer_c = priv->critic_normalizer;
    ch.privileged_observations = priv->privileged_observations; ch.last_observations = priv->last_observations;
  }
  if (ep) {
    if (!ep->raw_rewards || !ep->extras || !ep->cur_reward_sum || !ep->cur_episode_length || !ep->ep_return || !ep->ep_length)
      return lg_policy_fail(LG_ERR_INVALID, "null episode row");
    ch.raw_rewards = ep->raw_rewards; ch.extras = ep->extras;
  }
  int rc = lg_policy_collect_rollout(env, mem_a, actor, mem_c, critic, std, seed, first_call, T, gamma, lam, normalize_advantage, out, hid, h_a, c_a, h_c, c_c, &ch,
                                     stream);
  if (rc != LG_OK || !ep) return rc;
  EnvRewardRows rows;
  if ((rc = lg_policy_reward_rows(env, &rows)) != LG_OK) return rc;
  return lg_runner_episode_track(ep->raw_rewards, out->dones, T, rows.n, ep->cur_reward_sum, ep->cur_episode_length, ep->ep_return, ep->ep_length, stream);
}

extern "C" int lg_runner_collect(lg_ctx* env, lg_rnn* mem_a, lg_mlp* actor, lg_rnn* mem_c, lg_mlp* critic, const float* std, uint64_t seed, uint64_t first_call, int32_t T,
                                 float gamma, float lam, int32_t normalize_advantage, const lg_rollout* out, const lg_rollout_hidden* hid, float* h_a, float* c_a,
                                 float* h_c, float* c_c, const lg_runner_hooks* hooks, void* stream) {
  POLICY_ENTRY;
  return lg_runner_collect_both(env, mem_a, actor, mem_c, critic, std, seed, first_call, T, gamma, lam, normalize_advantage, out, hid, h_a, c_a, h_c, c_c, hooks, nullptr,
                                nullptr, stream);
}
