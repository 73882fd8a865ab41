// lg_planner.hip — gfx950 kernels of the sampling planner's arithmetic around rollout_batch (include/lgpolicy.h, section "the sampling planner"):
// node -> plan interpolation, the MPPI re-weighting, the samples of one diffusion pass, and the diffusion passes of one control step enqueued by one
// call.  Shares nothing with the network kernels of lg_policy.hip but the error channel (lg_policy_internal.h).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string>

#include "lg_device.h"
#include "lg_policy_internal.h"
#include "../../include/lgpolicy.h"
#include "../../include/lgstep.h"

// plans[i, h, a] = sum_k phi[h, k] nodes[i, k, a]: one lane per output element, the K node rows of a sample are read coalesced along a
__global__ __launch_bounds__(256) void plan_from_nodes_kernel(const float* __restrict__ nodes, const float* __restrict__ phi, int64_t n, int K, int H, int A,
                                                              float* __restrict__ plans) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n * H * A) return;
  const int a = (int)(idx % A); const int64_t ih = idx / A; const int h = (int)(ih % H); const int64_t i = ih / H;
  float acc = 0.f;
  for (int k = 0; k < K; ++k) acc = fmaf(phi[h * K + k], nodes[(i * K + k) * A + a], acc);
  plans[idx] = acc;
}

// One wave per main env: its R samples' mean rewards, standardised, softmax at the given temperature, weighted mean of the node rows.
// R, H, K * A are tens to hundreds: the whole problem of a main env is a few KB, read once.
__global__ __launch_bounds__(64) void mppi_update_kernel(const float* __restrict__ rewards, const float* __restrict__ nodes, int R, int H, int KA, float temperature,
                                                         float* __restrict__ new_nodes, float* __restrict__ weights) {
  extern __shared__ float w_lds[];                 // R weights
  const int m = blockIdx.x, lane = threadIdx.x;
  const float* rw = rewards + (size_t)m * R * H;
  auto wave_sum = [](float v) { for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o); return v; };
  auto wave_max = [](float v) { for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o)); return v; };
  float s1 = 0.f;
  for (int i = lane; i < R; i += 64) {
    float r = 0.f;
    for (int h = 0; h < H; ++h) r += rw[(size_t)i * H + h];
    r /= (float)H;
    w_lds[i] = r; s1 += r;
  }
  const float mean = wave_sum(s1) / (float)R;
  float s2 = 0.f;
  for (int i = lane; i < R; i += 64) { const float d = w_lds[i] - mean; s2 += d * d; }
  const float sd = sqrtf(wave_sum(s2) / (float)R);
  const float scale = sd > 1e-12f ? 1.f / (sd * temperature) : 0.f;
  float mx = -3.0e38f;
  for (int i = lane; i < R; i += 64) { const float z = (w_lds[i] - mean) * scale; w_lds[i] = z; mx = fmaxf(mx, z); }
  mx = wave_max(mx);
  float se = 0.f;
  for (int i = lane; i < R; i += 64) { const float e = __expf(w_lds[i] - mx); w_lds[i] = e; se += e; }
  const float inv = 1.f / wave_sum(se);
  for (int i = lane; i < R; i += 64) { const float w = w_lds[i] * inv; w_lds[i] = w; weights[(size_t)m * R + i] = w; }
  __syncthreads();
  const float* nd = nodes + (size_t)m * R * KA;
  for (int j = lane; j < KA; j += 64) {
    float acc = 0.f;
    for (int i = 0; i < R; ++i) acc = fmaf(w_lds[i], nd[(size_t)i * KA + j], acc);
    new_nodes[(size_t)m * KA + j] = acc;
  }
}

int lg_plan_from_nodes(const float* nodes, const float* phi, int64_t n, int32_t K, int32_t H, int32_t A, float* plans, void* stream) {
  POLICY_ENTRY;
  if (!nodes || !phi || !plans || n <= 0 || K <= 0 || H <= 0 || A <= 0) return lg_policy_fail(LG_ERR_INVALID, "null pointer or a size below 1");
  const int dev = lg_policy_device_of(nodes);
  if (dev < 0) return lg_policy_fail(LG_ERR_INVALID, "the nodes are not device memory");
  DeviceScope ds_(dev);
  const int64_t total = n * H * A;
  hipLaunchKernelGGL(plan_from_nodes_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, nodes, phi, n, K, H, A, plans);
  POLICY_TRY(hipGetLastError());
  return LG_OK;
}

int lg_mppi_update(const float* rewards, const float* nodes, int32_t num_main, int32_t R, int32_t H, int32_t K, int32_t A, float temperature,
                   float* new_nodes, float* weights, void* stream) {
  POLICY_ENTRY;
  if (!rewards || !nodes || !new_nodes || !weights || num_main <= 0 || R <= 0 || H <= 0 || K <= 0 || A <= 0 || !(temperature > 0.f))
    return lg_policy_fail(LG_ERR_INVALID, "null pointer, a size below 1 or a temperature that is not positive");
  if ((size_t)R * sizeof(float) > 60 * 1024) return lg_policy_fail(LG_ERR_UNSUPPORTED, "more than 15360 samples per main env");          // the weights of one main env live in LDS
  const int dev = lg_policy_device_of(rewards);
  if (dev < 0) return lg_policy_fail(LG_ERR_INVALID, "the rewards are not device memory");
  DeviceScope ds_(dev);
  hipLaunchKernelGGL(mppi_update_kernel, dim3((unsigned)num_main), dim3(64), (size_t)R * sizeof(float), (hipStream_t)stream, rewards, nodes, R, H, K * A, temperature,
                     new_nodes, weights);
  POLICY_TRY(hipGetLastError());
  return LG_OK;
}

// lg_mppi_sample_plans: one workgroup per sample row; the row's K x A nodes in LDS between the draw and the interpolation
__global__ __launch_bounds__(128) void mppi_sample_plans_kernel(const float* __restrict__ mean, const float* __restrict__ sigma_nodes, float sigma_scale,
                                                                const float* __restrict__ phi, int R, int K, int H, int A, uint32_t seed_lo, uint32_t seed_hi,
                                                                uint32_t call_lo, uint32_t call_hi, float* __restrict__ nodes, float* __restrict__ plans) {
  extern __shared__ float nd[];                      // [K * A]
  const int i = blockIdx.x, m = i / R, smp = i - m * R, KA = K * A;
  for (int j = threadIdx.x; j < KA; j += blockDim.x) {
    float z = 0.f;
    if (smp != 0) {
      uint32_t o[4];
      philox4((uint32_t)i, call_lo, (uint32_t)(j >> 1), call_hi, seed_lo, seed_hi, o);
      const float u1 = fmaxf(u01(o[0]), 5.9604645e-8f), u2 = u01(o[1]);
      const float rad = sqrtf(-2.f * logf(u1));
      z = (j & 1) ? rad * sinf(6.28318530717958647692f * u2) : rad * cosf(6.28318530717958647692f * u2);
    }
    const float v = mean[(size_t)m * KA + j] + (sigma_scale * sigma_nodes[j / A]) * z;
    nd[j] = v;
    nodes[(size_t)i * KA + j] = v;
  }
  __syncthreads();
  for (int j = threadIdx.x; j < H * A; j += blockDim.x) {
    const int h = j / A, a = j - h * A;
    float acc = 0.f;
    for (int k = 0; k < K; ++k) acc = fmaf(phi[h * K + k], nd[k * A + a], acc);
    plans[(size_t)i * H * A + j] = acc;
  }
}

int lg_mppi_sample_plans(const float* mean, const float* sigma_nodes, float sigma_scale, const float* phi, int32_t num_main, int32_t R, int32_t K, int32_t H,
                         int32_t A, uint64_t seed, uint64_t call, float* nodes, float* plans, void* stream) {
  POLICY_ENTRY;
  if (!mean || !sigma_nodes || !phi || !nodes || !plans || num_main <= 0 || R <= 0 || K <= 0 || H <= 0 || A <= 0) return lg_policy_fail(LG_ERR_INVALID, "null pointer or a size below 1");
  if ((size_t)K * A * sizeof(float) > 48 * 1024) return lg_policy_fail(LG_ERR_UNSUPPORTED, "more than 12288 node values (K x A) per sample");          // a sample's nodes live in LDS
  const int dev = lg_policy_device_of(mean);
  if (dev < 0) return lg_policy_fail(LG_ERR_INVALID, "the mean is not device memory");
  DeviceScope ds_(dev);
  hipLaunchKernelGGL(mppi_sample_plans_kernel, dim3((unsigned)(num_main * R)), dim3(128), (size_t)K * A * sizeof(float), (hipStream_t)stream, mean, sigma_nodes,
                     sigma_scale, phi, R, K, H, A, (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)call, (uint32_t)(call >> 32), nodes, plans);
  POLICY_TRY(hipGetLastError());
  return LG_OK;
}

// the diffusion passes of one control step, enqueued by one call (see lgpolicy.h)
int lg_planner_diffuse(lg_ctx* ctx, float* mean, const float* sigma_nodes, const float* phi, int32_t num_main, int32_t R, int32_t K, int32_t H, int32_t A,
                       int32_t n_diffuse, float traj_diffuse_factor, float temperature, uint64_t seed, uint64_t call0, const int32_t* env_ids,
                       int32_t rollouts_per_main, float pos_drift, float* nodes, float* plans, float* rewards, float* weights, void* stream) {
  POLICY_ENTRY;
  if (!ctx || !mean || !env_ids || !rewards || !weights || n_diffuse < 0 || rollouts_per_main != R)
    return lg_policy_fail(LG_ERR_INVALID, "null pointer, n_diffuse < 0, or rollouts_per_main is not R");
  float scale = 1.f;
  for (int pass = 0; pass < n_diffuse; ++pass) {
    int rc = lg_mppi_sample_plans(mean, sigma_nodes, scale, phi, num_main, R, K, H, A, seed, call0 + (uint64_t)pass, nodes, plans, stream);
    if (rc != LG_OK) return rc;
    rc = lg_rollout_batch(ctx, plans, H, env_ids, num_main * R, rollouts_per_main, pos_drift, rewards, stream);
    if (rc != LG_OK) return lg_policy_fail(rc, std::string("lg_rollout_batch failed: ") + lg_last_error(ctx));
    rc = lg_mppi_update(rewards, nodes, num_main, R, H, K, A, temperature, mean, weights, stream);      // (the update reads `nodes`, not `mean`: in place)
    if (rc != LG_OK) return rc;
    scale *= traj_diffuse_factor;
  }
  return LG_OK;
}
