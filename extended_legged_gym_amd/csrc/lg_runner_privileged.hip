// lg_runner_privileged.hip — the runner's collection with privileged critic observations (include/lgrunner_privileged.h): the paired normaliser
// step and the entry point of the two-stream collection (the one PPO loop in its two-stream mode: lg_policy.hip, lg_policy_collect_rollout; the
// entry body it shares with lg_runner_collect: lg_runner.hip).
//
// With two normalisers the collection loop would run lg_obsnorm_step twice per env step: six launches of a few microseconds each on a step of
// about a hundred.  The paired step runs each of the three phases as one launch over both handles: the grid's last index selects the handle, and
// a workgroup then runs the body the single kernel runs at the same (slab, column tile) -- lg_runner_internal.h -- on that handle's rows.  The
// two handles' widths differ (144 and 235 in anymal_c_rough_student: 3 and 4 column tiles), so the grid is as wide as the wider one and the
// workgroups past the narrower one's last tile leave at once.  Nothing is shared between the handles: no atomics, no workgroup waits on another.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>

#include "lg_device.h"
#include "lg_policy_internal.h"
#include "lg_runner_internal.h"
#include "../../include/lgpolicy.h"
#include "../../include/lgrunner.h"
#include "../../include/lgrunner_privileged.h"
#include "../../include/lgstep.h"

struct PartialSide { const float* x; int64_t stride; int O; double* partial; };
struct UpdateSide { const double* partial; int O; double rate; float *mean, *var, *sd; int64_t* count; int64_t new_count; };
struct ApplySide { const float* x; int64_t stride; int O; const float *mean, *sd; float eps; float* out; };

// grid (row slabs, column tiles of the wider handle, 2)
__global__ __launch_bounds__(ON_COLS * ON_WAVES) void obsnorm_partial_pair_kernel(PartialSide a, PartialSide c, int64_t n, int64_t slab_rows) {
  __shared__ double sh[3][ON_WAVES][ON_COLS];
  const PartialSide s = blockIdx.z ? c : a;
  if ((int)blockIdx.y * ON_COLS >= s.O) return;
  obsnorm_partial_body(sh, blockIdx.x, blockIdx.y, s.x, n, s.stride, s.O, slab_rows, s.partial);
}

// grid (column tiles of the wider handle, 2)
__global__ __launch_bounds__(ON_COLS * ON_UPD_WAVES) void obsnorm_update_pair_kernel(UpdateSide a, UpdateSide c, int slabs) {
  __shared__ double sh[3][ON_UPD_WAVES][ON_COLS];
  const UpdateSide s = blockIdx.y ? c : a;
  if ((int)blockIdx.x * ON_COLS >= s.O) return;
  obsnorm_update_body(sh, blockIdx.x, s.partial, slabs, s.O, s.rate, s.mean, s.var, s.sd, s.count, s.new_count);
}

// grid (column tiles of the wider handle, blocks of ON_APPLY_ROWS rows, 2)
__global__ __launch_bounds__(ON_COLS * ON_WAVES) void obsnorm_apply_pair_kernel(ApplySide a, ApplySide c, int64_t n) {
  const ApplySide s = blockIdx.z ? c : a;
  if ((int)blockIdx.x * ON_COLS >= s.O) return;
  obsnorm_apply_body(blockIdx.x, blockIdx.y, s.x, n, s.stride, s.O, s.mean, s.sd, s.eps, 0, s.out);
}

int lg_obsnorm_width(const lg_obsnorm* h) { return h->O; }

extern "C" {

int lg_obsnorm_step_pair(lg_obsnorm* h_a, const float* x_a, int64_t stride_a, float* out_a, lg_obsnorm* h_c, const float* x_c, int64_t stride_c, float* out_c,
                         int64_t n, int32_t update, void* stream) {
  POLICY_ENTRY;
  int rc = obsnorm_rows_ok(h_a, x_a, n, stride_a);
  if (rc == LG_OK) rc = obsnorm_rows_ok(h_c, x_c, n, stride_c);
  if (rc != LG_OK) return rc;
  if (h_a == h_c) return lg_policy_fail(LG_ERR_INVALID, "one normaliser given twice");
  if (h_a->device != h_c->device) return lg_policy_fail(LG_ERR_INVALID, "the two normalisers are on different devices");
  if (n == 0) return LG_OK;
  DeviceScope ds_(h_a->device);
  hipStream_t st = (hipStream_t)stream;
  const int tiles_a = (h_a->O + ON_COLS - 1) / ON_COLS, tiles_c = (h_c->O + ON_COLS - 1) / ON_COLS, tiles = tiles_a > tiles_c ? tiles_a : tiles_c;
  // each handle's freeze test is its own; a phase only one of them needs is that handle's single launch (lg_obsnorm_step makes the same test)
  const bool up_a = update && !(h_a->until >= 0 && h_a->count >= h_a->until), up_c = update && !(h_c->until >= 0 && h_c->count >= h_c->until);
  if (up_a && up_c) {
    int64_t slab_rows;
    const int slabs = obsnorm_slabs(n, &slab_rows);
    hipLaunchKernelGGL(obsnorm_partial_pair_kernel, dim3(slabs, tiles, 2), dim3(ON_COLS * ON_WAVES), 0, st, PartialSide{x_a, stride_a, h_a->O, h_a->partial},
                       PartialSide{x_c, stride_c, h_c->O, h_c->partial}, n, slab_rows);
    h_a->count += n; h_c->count += n;
    float *sa = h_a->state, *sc = h_c->state;
    hipLaunchKernelGGL(obsnorm_update_pair_kernel, dim3(tiles, 2), dim3(ON_COLS * ON_UPD_WAVES), 0, st,
                       UpdateSide{h_a->partial, h_a->O, (double)n / (double)h_a->count, sa, sa + h_a->O, sa + 2 * (size_t)h_a->O, h_a->count_dev, h_a->count},
                       UpdateSide{h_c->partial, h_c->O, (double)n / (double)h_c->count, sc, sc + h_c->O, sc + 2 * (size_t)h_c->O, h_c->count_dev, h_c->count}, slabs);
    POLICY_TRY(hipGetLastError());
  } else if (up_a) {
    rc = lg_obsnorm_step(h_a, x_a, n, stride_a, 1, nullptr, stream);
  } else if (up_c) {
    rc = lg_obsnorm_step(h_c, x_c, n, stride_c, 1, nullptr, stream);
  }
  if (rc != LG_OK) return rc;
  if (out_a && out_c) {
    hipLaunchKernelGGL(obsnorm_apply_pair_kernel, dim3(tiles, (unsigned)((n + ON_APPLY_ROWS - 1) / ON_APPLY_ROWS), 2), dim3(ON_COLS * ON_WAVES), 0, st,
                       ApplySide{x_a, stride_a, h_a->O, h_a->state, h_a->state + 2 * (size_t)h_a->O, h_a->eps, out_a},
                       ApplySide{x_c, stride_c, h_c->O, h_c->state, h_c->state + 2 * (size_t)h_c->O, h_c->eps, out_c}, n);
    POLICY_TRY(hipGetLastError());
  } else if (out_a) {
    rc = lg_obsnorm_step(h_a, x_a, n, stride_a, 0, out_a, stream);
  } else if (out_c) {
    rc = lg_obsnorm_step(h_c, x_c, n, stride_c, 0, out_c, stream);
  }
  return rc;
}

int lg_runner_collect_privileged(lg_ctx* env, lg_rnn* mem_a, lg_mlp* actor, lg_rnn* mem_c, lg_mlp* critic, const float* std, uint64_t seed, uint64_t first_call,
                                 int32_t T, float gamma, float lam, int32_t normalize_advantage, const lg_rollout* out, const lg_rollout_hidden* hid, float* h_a,
                                 float* c_a, float* h_c, float* c_c, const lg_runner_hooks* hooks, const lg_runner_privileged* priv, void* stream) {
  POLICY_ENTRY;
  if (!priv || !priv->privileged_observations) return lg_policy_fail(LG_ERR_INVALID, "null privileged struct or null privileged_observations rows");
  return lg_runner_collect_both(env, mem_a, actor, mem_c, critic, std, seed, first_call, T, gamma, lam, normalize_advantage, out, hid, h_a, c_a, h_c, c_c, hooks, priv,
                                nullptr, stream);
}

}  // extern "C"
