// lg_sensors.hip — the ray caster and the depth camera inside the one-call collectors (include/lgsensors.h): the sensor rig, the env step that
// drives the sensors between its two halves, the entry of the PPO collection over such a step (the one PPO loop: lg_policy.hip,
// lg_policy_collect_rollout with CollectHooks::sensors; the entry body it shares with lg_runner_collect: lg_runner.hip), and the estimation
// collection loop with its row gather.
//
// Nothing here casts a ray or steps a body: the launches are lg_step_physics, lg_raycaster_update_subset, the post-physics kernel with the
// transition sink and lg_depth_camera_update, in the order LeggedRobotDepth.step makes them from Python.  What this unit removes is the host
// between them: four ctypes calls, two Python method frames and the tensor bookkeeping of every env step of a collection.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>

#include "lg_bvh.h"
#include "lg_device.h"
#include "lg_estimator_internal.h"
#include "lg_policy_internal.h"
#include "lg_runner_internal.h"
#include "lg_runner_estimator_internal.h"
#include "../../include/lgpolicy.h"
#include "../../include/lgrunner.h"
#include "../../include/lgsensors.h"
#include "../../include/lgstep.h"

struct lg_sensor_rig {
  lg_ctx* env = nullptr;
  lg_mesh* mesh = nullptr;
  int device = 0;
  int64_t n = 0;                                   // envs of the context
  const float* root_states = nullptr;              // (n, 13), the context's
  const int64_t* episode_length_buf = nullptr;     // (n), the context's
  bool has_rays = false, has_camera = false;
  lg_sensor_raycaster rays{};
  lg_sensor_camera cam{};
  int64_t counter = 0;
  // scratch of lg_collect_estimation, allocated on its first call: the reward row nobody keeps, the actor's column prefix and its actions
  float* scratch = nullptr;
  size_t scratch_floats = 0;
};

// ---- the row gather of the estimation collection.  A streaming copy with twelve flops per target in it: one launch over three index ranges, in
// units of 16 bytes where the widths and the pointers allow (vec_depth: hw % 4 == 0; vec_tgt: groups of four consecutive (env, ray) pairs of the
// flat (n R) range, whose twelve hit floats are three aligned 16-byte loads), scalar units for the rest (the proprio rows: six floats from two
// tensors of row width three; the n R % 4 targets behind the last group).  Capped grid, grid-stride loop.
struct EstRowsArgs {
  const float* depth; int64_t frame_off, env_stride, hw; float* depth_out;          // frame_off: the newest frame inside an env's FIFO
  const float *lin, *ang; float* proprio_out;
  const float *hits, *root; int R; float* tgt_out;
  int64_t n, depth_units, proprio_units, tgt_groups, tgt_units;                      // tgt_units = groups + scalar tail
  int vec_depth, vec_tgt;
};

// |hit - root| in torch.norm's order of fp32 roundings over three components (measured against torch.norm(dim=2) on MI355X, 2.1 M vectors: the
// reduction pairs components 0 and 2 on one lane and adds component 1 from its neighbour): no contraction, a correctly rounded square root
__device__ __forceinline__ float est_target(float hx, float hy, float hz, float rx, float ry, float rz) {
#pragma clang fp contract(off)
  const float dx = hx - rx, dy = hy - ry, dz = hz - rz;
  const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
  const float s = xx + zz;
  return sqrtf(s + yy);
}

__global__ __launch_bounds__(256) void estimation_rows_kernel(EstRowsArgs a) {
#pragma clang fp contract(off)
  const int64_t total = a.depth_units + a.proprio_units + a.tgt_units;
  for (int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x; u < total; u += (int64_t)gridDim.x * 256) {
    if (u < a.depth_units) {
      if (a.vec_depth) {
        const int64_t per = a.hw >> 2, e = u / per, k = u - e * per;
        const float4 v = *reinterpret_cast<const float4*>(a.depth + e * a.env_stride + a.frame_off + 4 * k);
        *reinterpret_cast<float4*>(a.depth_out + e * a.hw + 4 * k) = v;
      } else {
        const int64_t e = u / a.hw, k = u - e * a.hw;
        a.depth_out[u] = a.depth[e * a.env_stride + a.frame_off + k];
      }
      continue;
    }
    int64_t v = u - a.depth_units;
    if (v < a.proprio_units) {
      const int64_t e = v / 6; const int j = (int)(v - e * 6);
      a.proprio_out[v] = j < 3 ? a.lin[e * 3 + j] : a.ang[e * 3 + j - 3];
      continue;
    }
    v -= a.proprio_units;
    if (v < a.tgt_groups) {
      const int64_t i0 = 4 * v;
      const float4* h = reinterpret_cast<const float4*>(a.hits + 3 * i0);
      const float4 h0 = h[0], h1 = h[1], h2 = h[2];
      const float hx[4] = {h0.x, h0.w, h1.z, h2.y}, hy[4] = {h0.y, h1.x, h1.w, h2.z}, hz[4] = {h0.z, h1.y, h2.x, h2.w};
      float o[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float* r = a.root + ((i0 + q) / a.R) * 13;
        o[q] = est_target(hx[q], hy[q], hz[q], r[0], r[1], r[2]);
      }
      *reinterpret_cast<float4*>(a.tgt_out + i0) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
      const int64_t i = (a.vec_tgt ? 4 * a.tgt_groups : 0) + (v - a.tgt_groups);
      const float* h = a.hits + 3 * i;
      const float* r = a.root + (i / a.R) * 13;
      a.tgt_out[i] = est_target(h[0], h[1], h[2], r[0], r[1], r[2]);
    }
  }
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

static int estimation_rows_launch(const float* depth_buffer, int32_t buffer_len, int64_t hw, const float* lin, const float* ang, const float* hits,
                                  const float* root, int64_t n, int32_t R, float* depth_out, float* proprio_out, float* tgt_out, hipStream_t st) {
  EstRowsArgs a{};
  a.n = n;
  if (depth_out) {
    a.depth = depth_buffer; a.hw = hw; a.env_stride = (int64_t)buffer_len * hw; a.frame_off = (int64_t)(buffer_len - 1) * hw; a.depth_out = depth_out;
    a.vec_depth = (hw & 3) == 0 && aligned16(depth_buffer) && aligned16(depth_out);
    a.depth_units = a.vec_depth ? n * (hw >> 2) : n * hw;
  }
  if (proprio_out) { a.lin = lin; a.ang = ang; a.proprio_out = proprio_out; a.proprio_units = n * 6; }
  if (tgt_out) {
    a.hits = hits; a.root = root; a.R = R; a.tgt_out = tgt_out;
    const int64_t total = n * R;
    a.vec_tgt = aligned16(hits) && aligned16(tgt_out);
    a.tgt_groups = a.vec_tgt ? total >> 2 : 0;
    a.tgt_units = a.tgt_groups + (total - 4 * a.tgt_groups);
  }
  const int64_t units = a.depth_units + a.proprio_units + a.tgt_units;
  if (units == 0) return LG_OK;
  const int64_t blocks = (units + 255) / 256;
  hipLaunchKernelGGL(estimation_rows_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, st, a);
  POLICY_TRY(hipGetLastError());
  return LG_OK;
}

// the sensor step behind its checks: lgsensors.h, lg_sensor_step_transition
static int sensor_step(lg_sensor_rig* rig, const float* actions, float* next_obs, const float* values, float gamma, float* rewards, float* dones, void* stream) {
  int rc = lg_step_physics(rig->env, actions, stream);
  if (rc != LG_OK) return lg_policy_fail(rc, std::string("lg_step_physics failed: ") + lg_last_error(rig->env));
  if (rig->has_rays) {
    const lg_sensor_raycaster& r = rig->rays;
    rc = lg_raycaster_update_subset(rig->mesh, rig->root_states, r.ray_origins, r.ray_dirs, r.num_rays, r.max_distance, r.attach_yaw_only, nullptr, (int32_t)rig->n,
                                    r.ray_hits, r.hits_found, r.raycast_distances, r.distance_stride, stream);
    if (rc != LG_OK) return lg_policy_fail(rc, std::string("lg_raycaster_update_subset failed: ") + lg_mesh_last_error(rig->mesh));
  }
  rc = lg_post_physics_transition(rig->env, next_obs, values, gamma, rewards, dones, stream);
  if (rc != LG_OK) return lg_policy_fail(rc, std::string("lg_post_physics_transition failed: ") + lg_last_error(rig->env));
  if (rig->has_camera) {
    const lg_sensor_camera& c = rig->cam;
    if (rig->counter % c.update_interval == 0) {
      rc = lg_depth_camera_update(rig->mesh, &c.params, rig->root_states, c.ray_dirs, rig->episode_length_buf, (int32_t)rig->n, nullptr, c.camera_pos, c.camera_rot,
                                  c.depth_buffer, stream);
      if (rc != LG_OK) return lg_policy_fail(rc, std::string("lg_depth_camera_update failed: ") + lg_mesh_last_error(rig->mesh));
    }
  }
  rig->counter += 1;
  return LG_OK;
}

// the loop's one call on a rig (lg_policy.hip): the rig's own device scope is the context's, which the loop has opened already
int lg_policy_sensor_step(lg_sensor_rig* rig, const float* actions, float* next_obs, const float* values, float gamma, float* rewards, float* dones, void* stream) {
  return sensor_step(rig, actions, next_obs, values, gamma, rewards, dones, stream);
}
lg_ctx* lg_policy_sensor_env(lg_sensor_rig* rig) { return rig->env; }

// The estimation collection loop behind lg_collect_estimation (a driver of actions or a bare actor, no stats) and lg_runner_collect_estimation
// (include/lgrunner_estimator.h): lg_runner_estimator_internal.h.  The policy's input row x is the env's raw row, its column prefix (a strided copy
// into scratch) when the policy is narrower, and the normaliser's output (scratch) when there is one.
int lg_estimation_collect(lg_sensor_rig* rig, const lg_estimation_driver* drv, int32_t T, const lg_estimation_out* out, const lg_estimation_nets* est,
                          const lg_estimation_stats* stats, void* stream) {
  if (!rig) return lg_policy_fail(LG_ERR_INVALID, "null sensor rig");
  if (!rig->has_rays || !rig->has_camera) return lg_policy_fail(LG_ERR_INVALID, "the rig must carry both the ray caster and the depth camera");
  if (T < 1) return lg_policy_fail(LG_ERR_INVALID, "T < 1");
  lg_mlp* actor = drv->actor; const float* actions = drv->actions;
  lg_rnn* mem = drv->memory; lg_obsnorm* norm = drv->normalizer;
  if ((actor != nullptr) == (actions != nullptr)) return lg_policy_fail(LG_ERR_INVALID, "exactly one of actor and actions must be given");
  if (!actor && (mem || norm)) return lg_policy_fail(LG_ERR_INVALID, "a memory or a normaliser needs the actor behind it: pre-drawn actions pass neither");
  if (!out || !out->depth_images || !out->proprio_data || !out->raycast_targets || !out->dones) return lg_policy_fail(LG_ERR_INVALID, "null output row");
  void* p; int64_t shp[4], ashp[4]; int32_t nd, dt;
  lg_ctx* env = rig->env;
  if (lg_get_tensor(env, LG_T_OBS_BUF, &p, shp, &nd, &dt) != LG_OK) return lg_policy_fail(LG_ERR_INVALID, std::string("the env's observation rows: ") + lg_last_error(env));
  const float* env_obs = (const float*)p; const int64_t n = rig->n, O = shp[1];
  if (lg_get_tensor(env, LG_T_ACTIONS, &p, ashp, &nd, &dt) != LG_OK) return lg_policy_fail(LG_ERR_INVALID, std::string("the env's action rows: ") + lg_last_error(env));
  const int64_t A = ashp[1];
  if (lg_get_tensor(env, LG_T_BASE_LIN_VEL, &p, shp, &nd, &dt) != LG_OK) return lg_policy_fail(LG_ERR_INVALID, std::string("the env's base_lin_vel: ") + lg_last_error(env));
  const float* lin = (const float*)p;
  if (lg_get_tensor(env, LG_T_BASE_ANG_VEL, &p, shp, &nd, &dt) != LG_OK) return lg_policy_fail(LG_ERR_INVALID, std::string("the env's base_ang_vel: ") + lg_last_error(env));
  const float* ang = (const float*)p;
  int64_t in_w = 0, mem_top = 0;
  if (actor) {
    int al, ain, aout, adev;
    lg_mlp_widths(actor, &al, &ain, &aout, &adev);
    if (adev != rig->device) return lg_policy_fail(LG_ERR_INVALID, "the actor is on another device than the env context");
    if (aout != A) return lg_policy_fail(LG_ERR_INVALID, "the actor ends in " + std::to_string(aout) + " actions, the env takes " + std::to_string(A));
    in_w = ain;
    if (mem) {
      int rtype, rin, rhid, rdev;
      lg_rnn_widths(mem, &rtype, &rin, &rhid, &rdev);
      if (rdev != rig->device) return lg_policy_fail(LG_ERR_INVALID, "the policy's memory is on another device than the env context");
      if (!drv->h || (rtype == LG_RNN_LSTM && !drv->c)) return lg_policy_fail(LG_ERR_INVALID, "the policy's memory needs its state (h, and c for an LSTM)");
      if (ain != rhid) return lg_policy_fail(LG_ERR_INVALID, "the actor reads " + std::to_string(ain) + " columns, the policy's memory has " + std::to_string(rhid) + " hidden units");
      in_w = rin;
      mem_top = (int64_t)(mem->num_layers - 1) * n * rhid;
    }
    if (in_w > O)
      return lg_policy_fail(LG_ERR_INVALID, std::string(mem ? "the policy's memory" : "the actor") + " reads " + std::to_string(in_w) + " columns, the env's observation row has " + std::to_string(O));
    if (norm) {
      if (norm->device != rig->device) return lg_policy_fail(LG_ERR_INVALID, "the normaliser is on another device than the env context");
      if (norm->O != in_w) return lg_policy_fail(LG_ERR_INVALID, "the normaliser has " + std::to_string(norm->O) + " columns, the policy reads " + std::to_string(in_w));
    }
  }
  const lg_depth_params& dp = rig->cam.params;
  const int64_t hw = (int64_t)dp.resized_width * dp.resized_height;
  const int R = rig->rays.num_rays;
  int64_t Rp = 0;
  if (est) {
    if (!est->encoder || !est->combine || !est->memory || !est->decoder || !est->h) return lg_policy_fail(LG_ERR_INVALID, "null estimator stage or memory state");
    if (!out->predictions) return lg_policy_fail(LG_ERR_INVALID, "null output row (predictions)");
    if (est->encoder->H != dp.resized_height || est->encoder->W != dp.resized_width)
      return lg_policy_fail(LG_ERR_INVALID, "the encoder takes " + std::to_string(est->encoder->H) + " x " + std::to_string(est->encoder->W) + " images, the camera's frames are " +
                                                std::to_string(dp.resized_height) + " x " + std::to_string(dp.resized_width));
    int cl, cin, cout, cdev, dl, din, dout, ddev, rtype, rin, rhid, rdev;
    lg_mlp_widths(est->combine, &cl, &cin, &cout, &cdev);
    lg_mlp_widths(est->decoder, &dl, &din, &dout, &ddev);
    lg_rnn_widths(est->memory, &rtype, &rin, &rhid, &rdev);
    if (cin - est->encoder->out_dim != 6) return lg_policy_fail(LG_ERR_INVALID, "the estimator's combination layer does not read the six base velocities behind the features");
    if (rtype == LG_RNN_LSTM && !est->c) return lg_policy_fail(LG_ERR_INVALID, "an LSTM needs its cell state");
    Rp = dout;
  }
  if (stats) {
    if (!est) return lg_policy_fail(LG_ERR_INVALID, "error figures need an estimator: stats without nets");
    if (Rp != R) return lg_policy_fail(LG_ERR_INVALID, "the estimator predicts " + std::to_string(Rp) + " distances, the ray caster has " + std::to_string(R) + " rays");
    const int rc = lg_estimation_stats_ok(stats, n, R);
    if (rc != LG_OK) return rc;
  }
  DeviceScope ds_(rig->device);
  hipStream_t st = (hipStream_t)stream;
  // scratch: [reward row n | the policy's input row n x in_w (a column prefix, or the normaliser's output) | its actions n x A]
  const bool prefix = actor && in_w < O;
  const bool own_row = prefix || norm;
  const size_t need = (size_t)n + (own_row ? (size_t)n * in_w : 0) + (actor ? (size_t)n * A : 0);
  if (need > rig->scratch_floats) {
    if (rig->scratch) { POLICY_TRY(hipStreamSynchronize(st)); (void)hipFree(rig->scratch); rig->scratch = nullptr; rig->scratch_floats = 0; }
    POLICY_TRY(hipMalloc((void**)&rig->scratch, need * sizeof(float)));
    rig->scratch_floats = need;
  }
  float* rew_row = rig->scratch;
  float* own = rig->scratch + n;
  float* act_row = own + (own_row ? (size_t)n * in_w : 0);
  int rc;
  for (int t = 0; t < T; ++t) {
    float* depth_t = out->depth_images + (size_t)t * n * hw;
    float* proprio_t = out->proprio_data + (size_t)t * n * 6;
    float* targets_t = out->raycast_targets + (size_t)t * n * R;
    float* dones_t = out->dones + (size_t)t * n;
    rc = estimation_rows_launch(rig->cam.depth_buffer, dp.buffer_len, hw, lin, ang, rig->rays.ray_hits, rig->root_states, n, R, depth_t, proprio_t, targets_t, st);
    if (rc != LG_OK) return rc;
    if (est) {
      float* pred_t = out->predictions + (size_t)t * n * Rp;
      rc = lg_estimator_step(est->encoder, est->combine, est->memory, est->decoder, depth_t, hw, proprio_t, n, est->h, est->c, nullptr, pred_t, stream);
      if (rc != LG_OK) return rc;
      if (stats && (rc = lg_estimation_errors_launch(pred_t, targets_t, n, R, stats, stats->mse + t, stats->mae + t, t == 0, st)) != LG_OK) return rc;
    }
    const float* act_t = actions ? actions + (size_t)t * n * A : act_row;
    if (actor) {
      const float* x = env_obs;
      if (prefix) {
        POLICY_TRY(hipMemcpy2DAsync(own, (size_t)in_w * 4, env_obs, (size_t)O * 4, (size_t)in_w * 4, (size_t)n, hipMemcpyDeviceToDevice, st));
        x = own;
      }
      if (norm) {
        if ((rc = lg_obsnorm_step(norm, x, n, in_w, 0, own, stream)) != LG_OK) return rc;
        x = own;
      }
      if (mem) {
        if ((rc = lg_rnn_step(mem, x, n, drv->h, drv->c, nullptr, nullptr, stream)) != LG_OK) return rc;
        x = drv->h + mem_top;
      }
      if ((rc = lg_mlp_forward(actor, x, n, act_row, stream)) != LG_OK) return rc;
    }
    if ((rc = sensor_step(rig, act_t, nullptr, nullptr, 0.f, rew_row, dones_t, stream)) != LG_OK) return rc;
    if (est && (rc = lg_rnn_reset_rows(est->memory, est->h, est->c, dones_t, n, stream)) != LG_OK) return rc;
    if (mem && (rc = lg_rnn_reset_rows(mem, drv->h, drv->c, dones_t, n, stream)) != LG_OK) return rc;
  }
  POLICY_TRY(hipGetLastError());
  return LG_OK;
}

extern "C" {

lg_sensor_rig* lg_sensor_rig_create(lg_ctx* env, lg_mesh* mesh, const lg_sensor_raycaster* rays, const lg_sensor_camera* cam) {
  POLICY_ENTRY;
  if (!env || !mesh) { lg_policy_fail(LG_ERR_INVALID, "null env context or mesh"); return nullptr; }
  if (!rays && !cam) { lg_policy_fail(LG_ERR_INVALID, "neither sensor given: a rig carries the ray caster, the depth camera, or both"); return nullptr; }
  void* p; int64_t shp[4]; int32_t nd, dt;
  if (lg_get_tensor(env, LG_T_ROOT_STATES, &p, shp, &nd, &dt) != LG_OK) { lg_policy_fail(LG_ERR_INVALID, std::string("the env's root states: ") + lg_last_error(env)); return nullptr; }
  lg_sensor_rig r;
  r.env = env; r.mesh = mesh; r.root_states = (const float*)p; r.n = shp[0];
  if (lg_get_tensor(env, LG_T_EPISODE_LENGTH_BUF, &p, shp, &nd, &dt) != LG_OK) { lg_policy_fail(LG_ERR_INVALID, std::string("the env's episode lengths: ") + lg_last_error(env)); return nullptr; }
  r.episode_length_buf = (const int64_t*)p;
  r.device = lg_policy_device_of(r.root_states);
  if (r.device < 0) { lg_policy_fail(LG_ERR_INVALID, "the env's root states are not device memory"); return nullptr; }
  if (mesh->device != r.device) {
    lg_policy_fail(LG_ERR_INVALID, "the mesh is on device " + std::to_string(mesh->device) + ", the env context on device " + std::to_string(r.device));
    return nullptr;
  }
  if (rays) {
    if (!rays->ray_origins || !rays->ray_dirs || !rays->ray_hits || !rays->hits_found || !rays->raycast_distances) { lg_policy_fail(LG_ERR_INVALID, "null ray-caster buffer"); return nullptr; }
    if (rays->num_rays < 1) { lg_policy_fail(LG_ERR_INVALID, "num_rays must be at least 1"); return nullptr; }
    if (rays->distance_stride < rays->num_rays) { lg_policy_fail(LG_ERR_INVALID, "the raycast_distances stride is smaller than num_rays"); return nullptr; }
    int32_t extra = 0;
    if (lg_extra_obs_info(env, &extra, nullptr) != LG_OK || extra != rays->num_rays) {
      lg_policy_fail(LG_ERR_INVALID, "the env context has num_extra_obs = " + std::to_string(extra) + ", the ray caster " + std::to_string(rays->num_rays) + " rays");
      return nullptr;
    }
    r.has_rays = true; r.rays = *rays;
  }
  if (cam) {
    if (!cam->ray_dirs || !cam->camera_pos || !cam->camera_rot || !cam->depth_buffer) { lg_policy_fail(LG_ERR_INVALID, "null depth-camera buffer"); return nullptr; }
    if (cam->update_interval < 1) { lg_policy_fail(LG_ERR_INVALID, "update_interval must be at least 1"); return nullptr; }
    if (cam->counter < 0) { lg_policy_fail(LG_ERR_INVALID, "the camera's step counter is negative"); return nullptr; }
    r.has_camera = true; r.cam = *cam; r.counter = cam->counter;
  }
  return new lg_sensor_rig(r);
}

void lg_sensor_rig_destroy(lg_sensor_rig* rig) {
  if (!rig) return;
  if (rig->scratch) { DeviceScope ds_(rig->device); (void)hipFree(rig->scratch); }
  delete rig;
}

int64_t lg_sensor_rig_counter(const lg_sensor_rig* rig) { return rig ? rig->counter : -1; }

int lg_sensor_rig_set_counter(lg_sensor_rig* rig, int64_t counter) {
  POLICY_ENTRY;
  if (!rig || counter < 0) return lg_policy_fail(LG_ERR_INVALID, "null rig or a negative counter");
  rig->counter = counter;
  return LG_OK;
}

int lg_sensor_step_transition(lg_sensor_rig* rig, const float* actions, float* next_observations, const float* values, float gamma, float* rewards, float* dones,
                              void* stream) {
  POLICY_ENTRY;
  if (!rig || !actions || !rewards || !dones) return lg_policy_fail(LG_ERR_INVALID, "null rig or row (actions, rewards, dones)");
  DeviceScope ds_(rig->device);
  return sensor_step(rig, actions, next_observations, values, gamma, rewards, dones, stream);
}

int lg_runner_collect_sensors(lg_sensor_rig* rig, lg_rnn* mem_a, lg_mlp* actor, lg_rnn* mem_c, lg_mlp* critic, const float* std, uint64_t seed, uint64_t first_call,
                              int32_t T, float gamma, float lam, int32_t normalize_advantage, const lg_rollout* out, const lg_rollout_hidden* hid, float* h_a, float* c_a,
                              float* h_c, float* c_c, const lg_runner_hooks* hooks, void* stream) {
  POLICY_ENTRY;
  if (!rig) return lg_policy_fail(LG_ERR_INVALID, "null sensor rig");
  return lg_runner_collect_both(rig->env, mem_a, actor, mem_c, critic, std, seed, first_call, T, gamma, lam, normalize_advantage, out, hid, h_a, c_a, h_c, c_c, hooks,
                                nullptr, rig, stream);
}

int lg_estimation_rows(const float* depth_buffer, int32_t buffer_len, int64_t hw, const float* base_lin_vel, const float* base_ang_vel, const float* ray_hits,
                       const float* root_states, int64_t n, int32_t R, float* depth_out, float* proprio_out, float* targets_out, void* stream) {
  POLICY_ENTRY;
  if (n < 1) return lg_policy_fail(LG_ERR_INVALID, "n must be at least 1");
  if (!depth_out && !proprio_out && !targets_out) return lg_policy_fail(LG_ERR_INVALID, "no output row");
  if (depth_out && (!depth_buffer || buffer_len < 1 || hw < 1)) return lg_policy_fail(LG_ERR_INVALID, "depth rows need the FIFO, buffer_len >= 1 and hw >= 1");
  if (proprio_out && (!base_lin_vel || !base_ang_vel)) return lg_policy_fail(LG_ERR_INVALID, "proprio rows need base_lin_vel and base_ang_vel");
  if (targets_out && (!ray_hits || !root_states || R < 1)) return lg_policy_fail(LG_ERR_INVALID, "target rows need ray_hits, root_states and R >= 1");
  const int dev = lg_policy_device_of(depth_out ? depth_out : (proprio_out ? proprio_out : targets_out));
  if (dev < 0) return lg_policy_fail(LG_ERR_INVALID, "the output rows are not device memory");
  DeviceScope ds_(dev);
  return estimation_rows_launch(depth_buffer, buffer_len, hw, base_lin_vel, base_ang_vel, ray_hits, root_states, n, R, depth_out, proprio_out, targets_out,
                                (hipStream_t)stream);
}

int lg_collect_estimation(lg_sensor_rig* rig, lg_mlp* actor, const float* actions, int32_t T, const lg_estimation_out* out, const lg_estimation_nets* est,
                          void* stream) {
  POLICY_ENTRY;
  lg_estimation_driver drv{};
  drv.actions = actions; drv.actor = actor;
  return lg_estimation_collect(rig, &drv, T, out, est, nullptr, stream);
}

}  // extern "C"
