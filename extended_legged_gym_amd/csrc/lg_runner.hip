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

#define ON_COLS 64          // columns per workgroup: one per lane
#define ON_WAVES 4          // row lanes of a workgroup
#define ON_MAX_SLABS 128    // row slabs at most: partials per column
#define ON_UNROLL 8         // rows a lane loads before it adds them

struct lg_obsnorm {
  int O = 0, device = 0;
  float eps = 0.f;
  int64_t until = -1;
  int64_t count = 0;                 // the host's copy of the device count: it decides whether an update is frozen and gives the rate
  float* state = nullptr;            // _mean, _var, _std: 3 x O
  int64_t* count_dev = nullptr;
  double* partial = nullptr;         // [slab][count, mean, M2][O]
  float* carried = nullptr;          // (carried_n, O)
  int64_t carried_n = 0;
  bool carried_valid = false;
};

// (count, mean, M2) of a and b -> a, the pairwise update (Chan, Golub, LeVeque 1979); b empty: a unchanged
LG_DEV void chan_merge(double& ca, double& ma, double& sa, double cb, double mb, double sb) {
  if (cb == 0.0) return;
  const double tot = ca + cb, d = mb - ma, f = cb / tot;          // (a may be empty: then a becomes b)
  ma += d * f;
  sa += sb + d * d * (ca * f);
  ca = tot;
}

__global__ __launch_bounds__(ON_COLS * ON_WAVES) void obsnorm_partial_kernel(const float* __restrict__ x, int64_t n, int64_t stride, int O, int64_t slab_rows,
                                                                             double* __restrict__ partial) {
  __shared__ double sh[3][ON_WAVES][ON_COLS];
  const int lane = threadIdx.x & (ON_COLS - 1), w = threadIdx.x / ON_COLS;
  const int col = blockIdx.y * ON_COLS + lane;
  const int64_t r0 = (int64_t)blockIdx.x * slab_rows;
  const int64_t r1 = r0 + slab_rows < n ? r0 + slab_rows : n;
  double cnt = 0.0, mean = 0.0, m2 = 0.0;
  if (col < O && r0 + w < r1) {
    const float* p = x + col;
    const double x0 = (double)p[(r0 + w) * stride];
    double s1 = 0.0, s2 = 0.0;
    for (int64_t r = r0 + w; r < r1; r += ON_WAVES * ON_UNROLL) {
      float v[ON_UNROLL];
#pragma unroll
      for (int k = 0; k < ON_UNROLL; ++k) {          // rows past the slab re-read its last row of this lane's and count for nothing
        const int64_t rk = r + (int64_t)k * ON_WAVES;
        v[k] = p[(rk < r1 ? rk : r) * stride];
      }
#pragma unroll
      for (int k = 0; k < ON_UNROLL; ++k) {
        if (r + (int64_t)k * ON_WAVES < r1) { const double d = (double)v[k] - x0; s1 += d; s2 += d * d; cnt += 1.0; }
      }
    }
    const double m = s1 / cnt;
    mean = x0 + m;
    m2 = s2 - s1 * m;
    if (m2 < 0.0) m2 = 0.0;
  }
  sh[0][w][lane] = cnt; sh[1][w][lane] = mean; sh[2][w][lane] = m2;
  __syncthreads();
  if (w == 0 && col < O) {
#pragma unroll
    for (int k = 1; k < ON_WAVES; ++k) chan_merge(cnt, mean, m2, sh[0][k][lane], sh[1][k][lane], sh[2][k][lane]);
    double* q = partial + (size_t)blockIdx.x * 3 * O;
    q[col] = cnt; q[O + col] = mean; q[2 * O + col] = m2;
  }
}

// 64 columns per workgroup of sixteen waves; wave w loads its run of <= ON_UPD_RUN slabs at once and merges it in slab order, the sixteen runs then
// merge pairwise through LDS (neighbours first: a fixed tree), and wave 0 applies the module's update in float64 on the f32 state, rounded once.
#define ON_UPD_WAVES 16
#define ON_UPD_RUN (ON_MAX_SLABS / ON_UPD_WAVES)
__global__ __launch_bounds__(ON_COLS * ON_UPD_WAVES) void obsnorm_update_kernel(const double* __restrict__ partial, int slabs, int O, double rate, float* mean,
                                                                                float* var, float* sd, int64_t* count, int64_t new_count) {
  __shared__ double sh[3][ON_UPD_WAVES][ON_COLS];
  const int lane = threadIdx.x & (ON_COLS - 1), w = threadIdx.x / ON_COLS;
  const int col = blockIdx.x * ON_COLS + lane;
  if (blockIdx.x == 0 && threadIdx.x == 0) *count = new_count;
  double pc[ON_UPD_RUN], pm[ON_UPD_RUN], ps[ON_UPD_RUN];
#pragma unroll
  for (int k = 0; k < ON_UPD_RUN; ++k) {
    const int g = w * ON_UPD_RUN + k;
    const bool live = col < O && g < slabs;
    const double* p = partial + (size_t)(live ? g : 0) * 3 * O + (live ? col : 0);
    pc[k] = live ? p[0] : 0.0; pm[k] = live ? p[O] : 0.0; ps[k] = live ? p[2 * (size_t)O] : 0.0;
  }
  double c = pc[0], m = pm[0], s = ps[0];
#pragma unroll
  for (int k = 1; k < ON_UPD_RUN; ++k) chan_merge(c, m, s, pc[k], pm[k], ps[k]);
  sh[0][w][lane] = c; sh[1][w][lane] = m; sh[2][w][lane] = s;
#pragma unroll
  for (int step = 1; step < ON_UPD_WAVES; step *= 2) {
    __syncthreads();
    if ((w & (2 * step - 1)) == 0) {
      chan_merge(c, m, s, sh[0][w + step][lane], sh[1][w + step][lane], sh[2][w + step][lane]);
      sh[0][w][lane] = c; sh[1][w][lane] = m; sh[2][w][lane] = s;
    }
  }
  if (w != 0 || col >= O) return;
  const double var_x = s / c, mean0 = (double)mean[col], var0 = (double)var[col];
  const double delta = m - mean0, mean1 = mean0 + rate * delta;
  const float var1 = (float)(var0 + rate * (var_x - var0 + delta * (m - mean1)));
  mean[col] = (float)mean1;
  var[col] = var1;
  sd[col] = (float)sqrt((double)var1);
}

// out = (x - mean) / (std + eps), or the inverse y * (std + eps) + mean: the module's f32 operations.  A workgroup is 64 columns by ON_APPLY_ROWS
// rows; a wave's lanes are adjacent columns, the four waves take every fourth row
#define ON_APPLY_ROWS 16
__global__ __launch_bounds__(ON_COLS * ON_WAVES) void obsnorm_apply_kernel(const float* x, int64_t n, int64_t stride, int O, const float* __restrict__ mean,
                                                                           const float* __restrict__ sd, float eps, int inverse, float* out) {
  const int col = blockIdx.x * ON_COLS + (threadIdx.x & (ON_COLS - 1)), w = threadIdx.x / ON_COLS;
  if (col >= O) return;
  const float m = mean[col], s = sd[col] + eps;
  const int64_t r0 = (int64_t)blockIdx.y * ON_APPLY_ROWS + w;
  float v[ON_APPLY_ROWS / ON_WAVES];
#pragma unroll
  for (int k = 0; k < ON_APPLY_ROWS / ON_WAVES; ++k) { const int64_t r = r0 + k * ON_WAVES; v[k] = r < n ? x[r * stride + col] : 0.f; }
#pragma unroll
  for (int k = 0; k < ON_APPLY_ROWS / ON_WAVES; ++k) {
    const int64_t r = r0 + k * ON_WAVES;
    if (r < n) out[r * stride + col] = inverse ? __fadd_rn(__fmul_rn(v[k], s), m) : (v[k] - m) / s;
  }
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

static int obsnorm_rows_ok(const lg_obsnorm* h, const float* x, int64_t n, int64_t row_stride) {
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
    int64_t slab_rows = (n + ON_MAX_SLABS - 1) / ON_MAX_SLABS;
    if (slab_rows < ON_WAVES) slab_rows = ON_WAVES;
    const int slabs = (int)((n + slab_rows - 1) / slab_rows);          // <= ON_MAX_SLABS, every slab holds a row
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

int lg_runner_collect(lg_ctx* env, lg_rnn* mem_a, lg_mlp* actor, lg_rnn* mem_c, lg_mlp* critic, const float* std, uint64_t seed, uint64_t first_call, int32_t T,
                      float gamma, float lam, int32_t normalize_advantage, const lg_rollout* out, const lg_rollout_hidden* hid, float* h_a, float* c_a, float* h_c,
                      float* c_c, const lg_runner_hooks* hooks, void* stream) {
  POLICY_ENTRY;
  if (!env || !actor || !critic || !std || !out || T <= 0) return lg_policy_fail(LG_ERR_INVALID, "null argument or T < 1");
  if ((mem_a != nullptr) != (mem_c != nullptr) || (mem_a && !hid)) return lg_policy_fail(LG_ERR_INVALID, "a recurrent policy needs both memories and the hidden-state rows");
  CollectHooks ch;
  const lg_runner_episode* ep = hooks ? hooks->episode : nullptr;
  if (hooks) { ch.normalizer = hooks->normalizer; ch.update = hooks->training != 0; }
  if (ep) {
    if (!ep->raw_rewards || !ep->extras || !ep->cur_reward_sum || !ep->cur_episode_length || !ep->ep_return || !ep->ep_length)
      return lg_policy_fail(LG_ERR_INVALID, "null episode row");
    ch.raw_rewards = ep->raw_rewards; ch.extras = ep->extras;
  }
  int rc = lg_policy_collect_rollout(env, mem_a, actor, mem_c, critic, std, seed, first_call, T, gamma, lam, normalize_advantage, out, hid, h_a, c_a, h_c, c_c,
                                     ch.normalizer || ep ? &ch : nullptr, stream);
  if (rc != LG_OK || !ep) return rc;
  void* p; int64_t shp[4]; int32_t nd, dt;
  if (lg_get_tensor(env, LG_T_REW_BUF, &p, shp, &nd, &dt) != LG_OK) return lg_policy_fail(LG_ERR_INVALID, std::string("the env's reward rows: ") + lg_last_error(env));
  return lg_runner_episode_track(ep->raw_rewards, out->dones, T, shp[0], ep->cur_reward_sum, ep->cur_episode_length, ep->ep_return, ep->ep_length, stream);
}

}  // extern "C"
