// lg_runner_internal.h — what lg_runner.hip (one normaliser per call) and lg_runner_privileged.hip (two per call) share: the normaliser handle
// and the bodies of its three kernels.  A body takes the workgroup's place in the grid (bx, by) as arguments, so that a kernel over two handles
// runs, in each of its workgroups, exactly the instructions the kernel over one handle runs there: the same slab boundaries, merge order and
// rounding points, hence the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "lg_device.h"
#include "../../include/lgrunner_privileged.h"

#define ON_COLS 64          // columns per workgroup: one per lane
#define ON_WAVES 4          // row lanes of a workgroup
#define ON_MAX_SLABS 128    // row slabs at most: partials per column
#define ON_UNROLL 8         // rows a lane loads before it adds them
#define ON_UPD_WAVES 16
#define ON_UPD_RUN (ON_MAX_SLABS / ON_UPD_WAVES)
#define ON_APPLY_ROWS 16

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

// the row slabs of an n-row batch: rows per slab and how many slabs (<= ON_MAX_SLABS, every slab holds a row)
static inline int obsnorm_slabs(int64_t n, int64_t* slab_rows) {
  int64_t r = (n + ON_MAX_SLABS - 1) / ON_MAX_SLABS;
  if (r < ON_WAVES) r = ON_WAVES;
  *slab_rows = r;
  return (int)((n + r - 1) / r);
}

// (count, mean, M2) of a and b -> a, the pairwise update (Chan, Golub, LeVeque 1979); b empty: a unchanged
LG_DEV void chan_merge(double& ca, double& ma, double& sa, double cb, double mb, double sb) {
  if (cb == 0.0) return;
  const double tot = ca + cb, d = mb - ma, f = cb / tot;          // (a may be empty: then a becomes b)
  ma += d * f;
  sa += sb + d * d * (ca * f);
  ca = tot;
}

// workgroup (bx = row slab, by = column tile) of the partial kernel; sh: the workgroup's LDS
LG_DEV void obsnorm_partial_body(double (*sh)[ON_WAVES][ON_COLS], int bx, int by, const float* __restrict__ x, int64_t n, int64_t stride, int O, int64_t slab_rows,
                                 double* __restrict__ partial) {
  const int lane = threadIdx.x & (ON_COLS - 1), w = threadIdx.x / ON_COLS;
  const int col = by * ON_COLS + lane;
  const int64_t r0 = (int64_t)bx * slab_rows;
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
    double* q = partial + (size_t)bx * 3 * O;
    q[col] = cnt; q[O + col] = mean; q[2 * O + col] = m2;
  }
}

// workgroup bx (a column tile) of the update kernel: 64 columns per workgroup of sixteen waves; wave w loads its run of <= ON_UPD_RUN slabs at once
// and merges it in slab order, the sixteen runs then merge pairwise through LDS (neighbours first: a fixed tree), and wave 0 applies the module's
// update in float64 on the f32 state, rounded once.
LG_DEV void obsnorm_update_body(double (*sh)[ON_UPD_WAVES][ON_COLS], int bx, const double* __restrict__ partial, int slabs, int O, double rate, float* mean,
                                float* var, float* sd, int64_t* count, int64_t new_count) {
  const int lane = threadIdx.x & (ON_COLS - 1), w = threadIdx.x / ON_COLS;
  const int col = bx * ON_COLS + lane;
  if (bx == 0 && threadIdx.x == 0) *count = new_count;
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

// workgroup (bx = column tile, by = block of ON_APPLY_ROWS rows) of the apply kernel: out = (x - mean) / (std + eps), or the inverse
// y * (std + eps) + mean: the module's f32 operations.  A wave's lanes are adjacent columns, the four waves take every fourth row
LG_DEV void obsnorm_apply_body(int bx, int by, const float* x, int64_t n, int64_t stride, int O, const float* __restrict__ mean, const float* __restrict__ sd,
                               float eps, int inverse, float* out) {
  const int col = bx * ON_COLS + (threadIdx.x & (ON_COLS - 1)), w = threadIdx.x / ON_COLS;
  if (col >= O) return;
  const float m = mean[col], s = sd[col] + eps;
  const int64_t r0 = (int64_t)by * ON_APPLY_ROWS + w;
  float v[ON_APPLY_ROWS / ON_WAVES];
#pragma unroll
  for (int k = 0; k < ON_APPLY_ROWS / ON_WAVES; ++k) { const int64_t r = r0 + k * ON_WAVES; v[k] = r < n ? x[r * stride + col] : 0.f; }
#pragma unroll
  for (int k = 0; k < ON_APPLY_ROWS / ON_WAVES; ++k) {
    const int64_t r = r0 + k * ON_WAVES;
    if (r < n) out[r * stride + col] = inverse ? __fadd_rn(__fmul_rn(v[k], s), m) : (v[k] - m) / s;
  }
}

// the checks every call over rows makes (lg_runner.hip): NULL handle, rows, stride, row count
int obsnorm_rows_ok(const lg_obsnorm* h, const float* x, int64_t n, int64_t row_stride);

// the body of lg_runner_collect (priv and sensors NULL), of lg_runner_collect_privileged and of lg_runner_collect_sensors (a rig: lg_sensors.hip), behind
// their POLICY_ENTRY (lg_runner.hip)
struct lg_sensor_rig;
int lg_runner_collect_both(lg_ctx* env, lg_rnn* mem_a, lg_mlp* actor, lg_rnn* mem_c, lg_mlp* critic, const float* std, uint64_t seed, uint64_t first_call, int32_t T,
                           float gamma, float lam, int32_t normalize_advantage, const lg_rollout* out, const lg_rollout_hidden* hid, float* h_a, float* c_a, float* h_c,
                           float* c_c, const lg_runner_hooks* hooks, const lg_runner_privileged* priv, lg_sensor_rig* sensors, void* stream);
