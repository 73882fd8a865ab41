// lg_runner_estimator.hip — the terrain-estimator runner's device side (include/lgrunner_estimator.h): the entry of the estimation collection loop
// with a driver (the loop itself: lg_sensors.hip, lg_estimation_collect, shared with lg_collect_estimation), and the error figures of `play`
// (rsl_rl runners/terrain_estimator_runner.py:666-670) with the per-ray sums beside them.
//
// The error figures are a column reduction of an (n, R) matrix that is read once: every lane owns a column unit, so a row is one coalesced read of
// the wave, nothing crosses lanes while the rows stream, and what is left to merge is small: four waves through LDS, at most EE_MAX_SLABS slabs
// through a workspace and a second launch.  No atomics and no workgroup waits on another: every order is fixed.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>

#include "lg_device.h"
#include "lg_policy_internal.h"
#include "lg_runner_estimator_internal.h"
#include "../../include/lgrunner_estimator.h"

#define EE_COLS 64           // column units per workgroup: one per lane
#define EE_WAVES 4           // row lanes of a workgroup
#define EE_MAX_SLABS 128     // row slabs at most: partials per ray
#define EE_MAX_R 65536
#define EE_FIN_THREADS 256

struct EstErrArgs {
  const float* pred; const float* tgt;      // (n, R)
  int64_t n; int R;
  int vec;                                  // a column unit is four adjacent rays, one 16-byte load per tensor; else one ray
  int units;                                // column units: R / 4 or R
  float* partial;                           // [slab][sq, abs, bias, max][R]
};

LG_DEV void ee_add(float d, float& sq, float& ab, float& bi, float& mx) {
  const float a = fabsf(d);
  sq += d * d; ab += a; bi += d; mx = fmaxf(mx, a);
}

// workgroup (x = row slab, y = tile of EE_COLS column units); slab x holds the rows 4 x + w + 4 gridDim.x k: the grid-stride loop of a capped grid
__global__ __launch_bounds__(EE_COLS * EE_WAVES) void estimation_error_kernel(EstErrArgs a) {
  __shared__ float sh[EE_WAVES - 1][4][4][EE_COLS];
  const int lane = threadIdx.x & (EE_COLS - 1), w = threadIdx.x / EE_COLS;
  const int unit = blockIdx.y * EE_COLS + lane;
  const bool live = unit < a.units;
  const int width = a.vec ? 4 : 1;
  float sq[4] = {0.f, 0.f, 0.f, 0.f}, ab[4] = {0.f, 0.f, 0.f, 0.f}, bi[4] = {0.f, 0.f, 0.f, 0.f}, mx[4] = {0.f, 0.f, 0.f, 0.f};
  if (live) {
    const int64_t step = (int64_t)gridDim.x * EE_WAVES;
    if (a.vec) {
      const float* p = a.pred + 4 * unit;
      const float* q = a.tgt + 4 * unit;
      for (int64_t r = (int64_t)blockIdx.x * EE_WAVES + w; r < a.n; r += step) {
        const float4 pv = *reinterpret_cast<const float4*>(p + r * a.R);
        const float4 tv = *reinterpret_cast<const float4*>(q + r * a.R);
        ee_add(pv.x - tv.x, sq[0], ab[0], bi[0], mx[0]);
        ee_add(pv.y - tv.y, sq[1], ab[1], bi[1], mx[1]);
        ee_add(pv.z - tv.z, sq[2], ab[2], bi[2], mx[2]);
        ee_add(pv.w - tv.w, sq[3], ab[3], bi[3], mx[3]);
      }
    } else {
      for (int64_t r = (int64_t)blockIdx.x * EE_WAVES + w; r < a.n; r += step)
        ee_add(a.pred[r * a.R + unit] - a.tgt[r * a.R + unit], sq[0], ab[0], bi[0], mx[0]);
    }
  }
  if (w > 0) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      sh[w - 1][0][j][lane] = sq[j]; sh[w - 1][1][j][lane] = ab[j]; sh[w - 1][2][j][lane] = bi[j]; sh[w - 1][3][j][lane] = mx[j];
    }
  }
  __syncthreads();
  if (w != 0 || !live) return;
#pragma unroll
  for (int k = 0; k < EE_WAVES - 1; ++k) {          // wave order: fixed
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      sq[j] += sh[k][0][j][lane]; ab[j] += sh[k][1][j][lane]; bi[j] += sh[k][2][j][lane]; mx[j] = fmaxf(mx[j], sh[k][3][j][lane]);
    }
  }
  float* out = a.partial + (size_t)blockIdx.x * 4 * a.R + (size_t)unit * width;
  if (a.vec) {          // (the workspace is 16-byte aligned in this mode, and R % 4 == 0)
    *reinterpret_cast<float4*>(out) = make_float4(sq[0], sq[1], sq[2], sq[3]);
    *reinterpret_cast<float4*>(out + a.R) = make_float4(ab[0], ab[1], ab[2], ab[3]);
    *reinterpret_cast<float4*>(out + 2 * (size_t)a.R) = make_float4(bi[0], bi[1], bi[2], bi[3]);
    *reinterpret_cast<float4*>(out + 3 * (size_t)a.R) = make_float4(mx[0], mx[1], mx[2], mx[3]);
  } else {
    out[0] = sq[0]; out[a.R] = ab[0]; out[2 * (size_t)a.R] = bi[0]; out[3 * (size_t)a.R] = mx[0];
  }
}

// one workgroup: per ray the slabs in ascending order, the four rows written (first) or updated; the step's two means from the rays' sums
__global__ __launch_bounds__(EE_FIN_THREADS) void estimation_error_finish_kernel(const float* __restrict__ partial, int slabs, int R, double inv_count, int first,
                                                                                 float* mse, float* mae, float* ray_sq, float* ray_abs, float* ray_bias,
                                                                                 float* ray_max) {
  __shared__ double sh[2][EE_FIN_THREADS];
  double tot_sq = 0.0, tot_ab = 0.0;
  for (int c = threadIdx.x; c < R; c += EE_FIN_THREADS) {
    float s = 0.f, b = 0.f, d = 0.f, m = 0.f;
    const float* p = partial + c;
#pragma unroll 8
    for (int k = 0; k < slabs; ++k) {
      const float* q = p + (size_t)k * 4 * R;
      s += q[0]; b += q[R]; d += q[2 * (size_t)R]; m = fmaxf(m, q[3 * (size_t)R]);
    }
    tot_sq += (double)s; tot_ab += (double)b;
    if (first) { ray_sq[c] = s; ray_abs[c] = b; ray_bias[c] = d; ray_max[c] = m; }
    else { ray_sq[c] += s; ray_abs[c] += b; ray_bias[c] += d; ray_max[c] = fmaxf(ray_max[c], m); }
  }
  sh[0][threadIdx.x] = tot_sq; sh[1][threadIdx.x] = tot_ab;
#pragma unroll
  for (int step = EE_FIN_THREADS / 2; step > 0; step >>= 1) {          // a fixed tree
    __syncthreads();
    if ((int)threadIdx.x < step) { sh[0][threadIdx.x] += sh[0][threadIdx.x + step]; sh[1][threadIdx.x] += sh[1][threadIdx.x + step]; }
  }
  if (threadIdx.x == 0) { *mse = (float)(sh[0][0] * inv_count); *mae = (float)(sh[1][0] * inv_count); }
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

static int ee_slabs(int64_t n) {
  const int64_t s = (n + EE_WAVES - 1) / EE_WAVES;
  return (int)(s < EE_MAX_SLABS ? s : EE_MAX_SLABS);
}

int lg_estimation_stats_ok(const lg_estimation_stats* s, int64_t n, int32_t R) {
  if (!s->mse || !s->mae || !s->ray_sq_error || !s->ray_abs_error || !s->ray_bias || !s->ray_max_error || !s->workspace)
    return lg_policy_fail(LG_ERR_INVALID, "null member of the error figures (mse, mae, the four per-ray rows, workspace)");
  const int64_t need = lg_estimation_errors_workspace(n, R);
  if (need < 0) return lg_policy_fail(LG_ERR_INVALID, "n must be at least 1 and R in 1.." + std::to_string(EE_MAX_R));
  if (s->workspace_floats < need)
    return lg_policy_fail(LG_ERR_INVALID, "the workspace holds " + std::to_string(s->workspace_floats) + " floats, " + std::to_string(n) + " rows of " + std::to_string(R) +
                                              " rays need " + std::to_string(need));
  return LG_OK;
}

int lg_estimation_errors_launch(const float* pred, const float* tgt, int64_t n, int32_t R, const lg_estimation_stats* s, float* mse, float* mae, int first,
                                hipStream_t st) {
  EstErrArgs a{};
  a.pred = pred; a.tgt = tgt; a.n = n; a.R = R; a.partial = s->workspace;
  a.vec = (R & 3) == 0 && aligned16(pred) && aligned16(tgt) && aligned16(s->workspace);
  a.units = a.vec ? R >> 2 : R;
  const int slabs = ee_slabs(n);
  hipLaunchKernelGGL(estimation_error_kernel, dim3((unsigned)slabs, (unsigned)((a.units + EE_COLS - 1) / EE_COLS)), dim3(EE_COLS * EE_WAVES), 0, st, a);
  hipLaunchKernelGGL(estimation_error_finish_kernel, dim3(1), dim3(EE_FIN_THREADS), 0, st, (const float*)s->workspace, slabs, (int)R,
                     1.0 / ((double)n * (double)R), first, mse, mae, s->ray_sq_error, s->ray_abs_error, s->ray_bias, s->ray_max_error);
  POLICY_TRY(hipGetLastError());
  return LG_OK;
}

extern "C" {

int64_t lg_estimation_errors_workspace(int64_t n, int32_t R) {
  if (n < 1 || R < 1 || R > EE_MAX_R) return LG_ERR_INVALID;
  return (int64_t)ee_slabs(n) * 4 * R;
}

int lg_estimation_errors(const float* predictions, const float* targets, int32_t steps, int64_t n, int32_t R, const lg_estimation_stats* stats, void* stream) {
  POLICY_ENTRY;
  if (!predictions || !targets || !stats) return lg_policy_fail(LG_ERR_INVALID, "null predictions, targets or stats");
  if (steps < 1 || n < 1 || R < 1 || R > EE_MAX_R) return lg_policy_fail(LG_ERR_INVALID, "steps and n must be at least 1 and R in 1.." + std::to_string(EE_MAX_R));
  int rc = lg_estimation_stats_ok(stats, n, R);
  if (rc != LG_OK) return rc;
  const int dev = lg_policy_device_of(predictions);
  if (dev < 0) return lg_policy_fail(LG_ERR_INVALID, "the predictions are not device memory");
  DeviceScope ds_(dev);
  for (int32_t t = 0; t < steps; ++t) {
    const size_t off = (size_t)t * n * R;
    if ((rc = lg_estimation_errors_launch(predictions + off, targets + off, n, R, stats, stats->mse + t, stats->mae + t, t == 0, (hipStream_t)stream)) != LG_OK) return rc;
  }
  return LG_OK;
}

int lg_runner_collect_estimation(lg_sensor_rig* rig, const lg_estimation_driver* driver, int32_t T, const lg_estimation_out* out, const lg_estimation_nets* nets,
                                 const lg_estimation_stats* stats, void* stream) {
  POLICY_ENTRY;
  if (!driver) return lg_policy_fail(LG_ERR_INVALID, "null driver");
  if (driver->critic) return lg_policy_fail(LG_ERR_INVALID, "a critic: the estimation collection reads no value, the driver is the actor alone");
  if (driver->std) return lg_policy_fail(LG_ERR_INVALID, "sampling (std): the driver is the deterministic act_inference");
  if (driver->normalizer && driver->normalizer_training)
    return lg_policy_fail(LG_ERR_INVALID, "a normaliser in training mode: the driver's statistics do not move during estimator training");
  if (driver->privileged_observations) return lg_policy_fail(LG_ERR_INVALID, "two observation streams: the driver reads the env's one row");
  if (driver->memory && !driver->actor) return lg_policy_fail(LG_ERR_INVALID, "a memory without the actor that reads it");
  return lg_estimation_collect(rig, driver, T, out, nets, stats, stream);
}

}  // extern "C"
