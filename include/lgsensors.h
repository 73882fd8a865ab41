/* lgsensors.h — C ABI of the perception sensors INSIDE the one-call collectors: the ray caster and the ray-cast depth camera of
 * LeggedRobotRayCast / LeggedRobotDepth (reference envs/base/legged_robot_raycast.py:219-260, legged_robot_depthcam.py:110-129) attached to an env
 * context as a SENSOR RIG, the env step that drives them between its two halves, the PPO collection of lgrunner.h over such a step, and the
 * data-collection loop of TerrainEstimatorRunner.learn (rsl_rl runners/terrain_estimator_runner.py:392-438) as one call.
 * Same library and conventions as lgpolicy.h / lgrunner.h; every refusal leaves its message on their error channel (lg_mlp_last_error), with
 * nothing launched.  Device pointers unless marked HOST; every launch is asynchronous on the caller's hipStream_t.  No sensor, physics or policy
 * kernel is new: the one kernel of this unit is the row gather of lg_estimation_rows.  Equal inputs give equal bits. */
#ifndef LGSENSORS_H
#define LGSENSORS_H
#include <stdint.h>
#include "lgstep.h"
#include "lgpolicy.h"
#include "lgrunner.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- two step entry points of the env context, beside lg_step_physics and lg_set_extra_obs of lgstep.h (dispatched per topology like them).
 * lg_post_physics_transition: the second half of lg_step_transition -- lg_post_physics_step whose kernel also writes the new observation rows to
 * next_observations (may be NULL), rewards[k] = rew + gamma * values[k] * time_out (values NULL: rew) and dones[k].  Pairs with lg_step_physics.
 * lg_extra_obs_info: lg_config.num_extra_obs of the context and the buffer lg_set_extra_obs bound (NULL: none); either output may be NULL. */
int lg_post_physics_transition(lg_ctx* ctx, float* next_observations, const float* values, float gamma, float* rewards, float* dones, void* stream);
int lg_extra_obs_info(lg_ctx* ctx, int32_t* num_extra_obs, const float** bound);

/* ---- the sensor rig */
typedef struct lg_sensor_raycaster {
  const float* ray_origins;        /* (num_rays, 3) pattern origins, base frame (offset_pos added) */
  const float* ray_dirs;           /* (num_rays, 3) pattern directions */
  int32_t num_rays;
  float max_distance;
  int32_t attach_yaw_only;
  float* ray_hits;                 /* (N, num_rays, 3) */
  uint8_t* hits_found;             /* (N, num_rays) */
  float* raycast_distances;        /* row e at raycast_distances + e * distance_stride: the buffer bound with lg_set_extra_obs */
  int32_t distance_stride;         /* >= num_rays */
} lg_sensor_raycaster;

typedef struct lg_sensor_camera {
  lg_depth_params params;
  const float* ray_dirs;           /* (height * width, 3) pixel rays */
  float* camera_pos;               /* (N, 3) */
  float* camera_rot;               /* (N, 4) */
  float* depth_buffer;             /* (N, buffer_len, resized_height, resized_width): the frame FIFO */
  int32_t update_interval;         /* >= 1: the camera updates on the steps whose counter is a multiple of it */
  int64_t counter;                 /* the env's depth_update_counter when the rig is made */
} lg_sensor_camera;

typedef struct lg_sensor_rig lg_sensor_rig;

/* The sensors of one env context: the ray caster, the camera, or both (the other NULL), casting against `mesh`.  The rig reads root_states and
 * episode_length_buf from the context (lg_get_tensor) and OWNS NO SENSOR MEMORY: every buffer above stays the caller's, so after any call on the
 * rig the caller's tensors hold what they would hold after the env class's own step.  Context, mesh and buffers must outlive the rig.
 * NULL + a message: env or mesh NULL; neither sensor given; a NULL buffer; num_rays < 1; update_interval < 1; a mesh on another device than the
 * context; distance_stride < num_rays; with the ray caster, a context whose num_extra_obs is not num_rays. */
lg_sensor_rig* lg_sensor_rig_create(lg_ctx* env, lg_mesh* mesh, const lg_sensor_raycaster* raycaster, const lg_sensor_camera* camera);
void lg_sensor_rig_destroy(lg_sensor_rig* rig);
/* The camera's step counter (depth_update_counter): every sensor step adds one.  get: -1 for a NULL rig.  set: when the env was stepped from
 * the host between two calls on the rig. */
int64_t lg_sensor_rig_counter(const lg_sensor_rig* rig);
int lg_sensor_rig_set_counter(lg_sensor_rig* rig, int64_t counter);

/* LeggedRobotDepth.step with the transition sink of lg_step_transition, launch for launch in the env class's order:
 *   1. lg_step_physics(actions)
 *   2. the ray caster on all envs, from the post-physics, pre-reset base pose (lg_raycaster_update_subset, env_ids NULL)      [rig with rays]
 *   3. lg_post_physics_transition(next_observations, values, gamma, rewards, dones): the distance rows enter the observation here
 *   4. when counter % update_interval == 0: lg_depth_camera_update from the post-reset pose and episode_length_buf; then counter += 1  [camera]
 * next_observations and values may be NULL.  Refused: NULL rig, actions, rewards or dones. */
int lg_sensor_step_transition(lg_sensor_rig* rig, const float* actions, float* next_observations, const float* values, float gamma, float* rewards,
                              float* dones, void* stream);

/* lg_runner_collect (lgrunner.h) on an env whose step is lg_sensor_step_transition: the one PPO collection loop with that call in the place of
 * lg_step_transition and nothing else moved -- feed-forward (mem_a, mem_c, hid and the four state pointers NULL) and recurrent, hooks as there.
 * hooks NULL or both members NULL: the rows of lg_collect_rollout / lg_collect_rollout_recurrent, so THIS is also the plain collector with a rig;
 * there is no separate lg_collect_rollout_sensors.  Privileged critic observations (two streams) have no rig variant.
 * Refused: rig NULL, and everything lg_runner_collect refuses. */
int lg_runner_collect_sensors(lg_sensor_rig* rig, lg_rnn* mem_a, lg_mlp* actor, lg_rnn* mem_c, lg_mlp* critic, const float* std, uint64_t seed,
                              uint64_t first_call, int32_t T, float gamma, float lam, int32_t normalize_advantage, const lg_rollout* out,
                              const lg_rollout_hidden* hid, float* h_a, float* c_a, float* h_c, float* c_c, const lg_runner_hooks* hooks, void* stream);

/* ---- estimation collection.
 * One row of TerrainEstimatorRunner._get_environment_data (terrain_estimator_runner.py:247-277) for n envs, ONE launch (a streaming copy: 16-byte
 * accesses where a row's width and the pointers allow them, scalar otherwise):
 *   depth_out   (n, hw)  = the newest frame of the FIFO depth_buffer (n, buffer_len, hw)
 *   proprio_out (n, 6)   = base_lin_vel (n, 3) | base_ang_vel (n, 3)
 *   targets_out (n, R)   = |ray_hits (n, R, 3) - root_states[:, 0:3]| (root_states: (n, 13)), in torch.norm's fp32 order:
 *                          d = hit - root (rounded), sqrt((dx dx + dz dz) + dy dy), every product and sum rounded, no fused multiply-add
 * Any of the three outputs may be NULL (that part is skipped).  Refused: a NULL input of a requested part, n < 1, hw / R / buffer_len < 1. */
int lg_estimation_rows(const float* depth_buffer, int32_t buffer_len, int64_t hw, const float* base_lin_vel, const float* base_ang_vel,
                       const float* ray_hits, const float* root_states, int64_t n, int32_t R, float* depth_out, float* proprio_out, float* targets_out,
                       void* stream);

typedef struct lg_estimation_out {
  float* depth_images;             /* (T, n, resized_height, resized_width) */
  float* proprio_data;             /* (T, n, 6) */
  float* raycast_targets;          /* (T, n, num_rays) */
  float* dones;                    /* (T, n) */
  float* predictions;              /* (T, n, decoder width); read only with an estimator */
} lg_estimation_out;

typedef struct lg_estimation_nets {          /* the four stages of lg_estimator_step (lgpolicy.h) and the memory's live state */
  lg_conv_encoder* encoder;
  lg_mlp* combine;
  lg_rnn* memory;
  lg_mlp* decoder;
  float* h;                        /* (L, n, H), in place */
  float* c;                        /* an LSTM's cell state; NULL for a GRU */
} lg_estimation_nets;

/* The collection loop of TerrainEstimatorRunner.learn over an env with both sensors, without returning to the host.  Per step t:
 *   rows       lg_estimation_rows into row t of the three tensors, from the state the previous step left (t = 0: the state at entry).  The
 *              targets keep the host loop's quirk: the hits are from the pre-reset pose, the root position from after the reset;
 *   estimator  (est not NULL) lg_estimator_step on row t into predictions[t], no reset row;
 *   actions    actor not NULL: lg_mlp_forward on the env's raw observation row -- an actor narrower than the row reads its column prefix (a strided
 *              copy), a wide actor (lgpolicy_wide.h) the wide forward; actor NULL: row t of `actions` (T, n, A).  Exactly one of the two;
 *   step       lg_sensor_step_transition without a value row; dones[t] is the step's done row, reward and next-observation rows are not kept;
 *   memory     (est not NULL) lg_rnn_reset_rows on dones[t].
 * Refused: rig NULL or without BOTH sensors; T < 1; both or neither of actor / actions; a NULL output row (predictions with est); an actor wider
 * than the env's row or not ending in one action per DOF; est with a NULL stage or state, or whose encoder does not take the camera's frame. */
int lg_collect_estimation(lg_sensor_rig* rig, lg_mlp* actor, const float* actions, int32_t T, const lg_estimation_out* out,
                          const lg_estimation_nets* est, void* stream);

#ifdef __cplusplus
}
#endif
#endif
