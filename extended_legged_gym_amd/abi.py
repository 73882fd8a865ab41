"""ctypes mirror of the headers under `include/` (the C ABI of the env-step library).

Only declarations live here: struct layouts, enum values and function prototypes, one `declare_*` function per unit, and at the
end the table of units (`UNITS`) with `declare(lib, *units)`, the one way to set prototypes on a library.  `tests/test_abi_units.py`
parses every header and checks names, exports and struct layouts against this file, `tests/test_abi.py` the enum values, so the
two cannot drift apart.
"""
import collections
import ctypes as C
import functools
import types

LG_ABI_VERSION = 5
LG_MAX_LEGS, LG_JOINTS_PER_LEG, LG_MAX_JOINTS_PER_LEG = 6, 3, 6
LG_MAX_DOF = 18
LG_MAX_CP, LG_MAX_BODIES, LG_MAX_REWARD_TERMS, LG_MAX_INDEX_LIST = 8, 25, 32, 25
LG_MAX_SC_PAIRS = 96
SUPPORTED_LEG_COUNTS = (4, 6, 2)       # kernel instances of the library (csrc/lg_instance.h): 4 x 3, 6 x 3, 2 x 6 joints
JOINTS_PER_LEG_OF = {4: 3, 6: 3, 2: 6}
LG_LSTM_NPARAM = 969

LG_OK, LG_ERR_INVALID, LG_ERR_HIP, LG_ERR_UNSUPPORTED, LG_ERR_NO_DEVICE = 0, -1, -2, -3, -4
LG_F32, LG_I64, LG_U8, LG_I16, LG_I32, LG_F64 = 0, 1, 2, 3, 4, 5
LG_CTRL_P, LG_CTRL_V, LG_CTRL_T, LG_CTRL_ACTUATOR_NET = 0, 1, 2, 3
LG_MESH_PLANE, LG_MESH_HEIGHTFIELD, LG_MESH_TRIMESH = 0, 1, 2
LG_RNG_PHILOX, LG_RNG_INJECT = 0, 1
LG_SOLVER_PGS, LG_SOLVER_TGS = 0, 1
LG_FRICTION_CONE, LG_FRICTION_PYRAMID = 0, 1


def rand_slots(num_dof=12):
    """Slots of the per-env uniform-draw table (enum lg_rand_slot + the LG_RS_*_OF(dof) macros of lgstep.h)."""
    root_xy = 8 + num_dof
    return dict(LG_RS_CMD_CB=0, LG_RS_PUSH=4, LG_RS_LEVEL=6, LG_RS_DOF=8, LG_RS_ROOT_XY=root_xy, LG_RS_ROOT_VEL=root_xy + 2,
                LG_RS_CMD_RESET=root_xy + 8, LG_RS_NOISE=(root_xy + 8 + 3 + 3) & ~3)


def num_proprio(num_dof=12):
    """Observation entries in front of the height scan (LG_NUM_PROPRIO_OF): 48 for 12 DOF, 66 for 18."""
    return 12 + 3 * num_dof


RAND_SLOTS = rand_slots(12)            # the four-legged robots' table (20 / 22 / 28 / 32)
LG_RS_NOISE = RAND_SLOTS["LG_RS_NOISE"]

# reward term name (as in cfg.rewards.scales) -> lg_reward_term
REWARD_TERMS = [
    "action_rate", "ang_vel_xy", "base_foot_height", "base_height", "collision", "dof_acc", "dof_pos_limits", "dof_vel",
    "dof_vel_limits", "feet_air_time", "feet_contact_forces", "feet_slip", "feet_stumble", "feet_stumble_liftup",
    "four_footup", "gait_2_step", "gait_scheduler", "jump_air", "lin_vel_z", "orientation", "stand_still", "termination",
    "torque_limits", "torques", "tracking_ang_vel", "tracking_lin_vel",
    # class-specific variants: selected through an env class's `reward_term_variants`, never named in a config
    "orientation_load_adapt",
    # StandAnymal / StandGo2 only (anymal.py:301-308); the other overrides of those classes come with lg_config.reward_class
    "penalty_in_the_air", "async_gait_scheduler",
    "no_fly"]                                              # Cassie (cassie.py:42-45)
REWARD_CLASSES = {"base": 0, "stand": 1}                   # enum lg_reward_class
REWARD_TERM_ID = {n: i for i, n in enumerate(REWARD_TERMS)}

TENSOR_NAMES = [
    "root_states", "dof_state", "rigid_body_state", "contact_forces", "torques", "actions", "last_actions", "last_dof_vel",
    "last_root_vel", "commands", "base_lin_vel", "base_ang_vel", "projected_gravity", "base_lin_acc", "base_ang_acc",
    "feet_air_time", "feet_contact_time", "last_contacts", "measured_heights", "obs_buf", "rew_buf", "reset_buf",
    "time_out_buf", "episode_length_buf", "episode_sums", "terrain_levels", "terrain_types", "env_origins",
    "friction_coeffs", "base_mass_added", "sea_hidden_state", "sea_cell_state", "gait_idx", "gait_foot_z",
    "extras_episode", "rand_inject", "step_counters", "height_samples", "terrain_origins", "episode_stats", "command_ranges"]
TENSOR_ID = {n: i for i, n in enumerate(TENSOR_NAMES)}
LG_T_COUNT = len(TENSOR_NAMES)

f32, i32 = C.c_float, C.c_int32


class lg_robot_model(C.Structure):
    _fields_ = [
        ("num_legs", i32), ("num_joints_per_leg", i32), ("num_bodies", i32), ("has_foot_body", i32),
        ("base_mass", f32), ("base_com", f32 * 3), ("base_inertia", f32 * 6),
        ("joint_pos", (f32 * 3) * LG_MAX_JOINTS_PER_LEG * LG_MAX_LEGS), ("joint_rot", (f32 * 9) * LG_MAX_JOINTS_PER_LEG * LG_MAX_LEGS),
        ("joint_axis", (f32 * 3) * LG_MAX_JOINTS_PER_LEG * LG_MAX_LEGS),
        ("link_mass", (f32 * LG_MAX_JOINTS_PER_LEG) * LG_MAX_LEGS), ("link_com", (f32 * 3) * LG_MAX_JOINTS_PER_LEG * LG_MAX_LEGS),
        ("link_inertia", (f32 * 6) * LG_MAX_JOINTS_PER_LEG * LG_MAX_LEGS),
        ("foot_pos", (f32 * 3) * LG_MAX_LEGS), ("foot_rot", (f32 * 9) * LG_MAX_LEGS),
        ("dof_lower", f32 * LG_MAX_DOF), ("dof_upper", f32 * LG_MAX_DOF), ("dof_vel_limit", f32 * LG_MAX_DOF), ("torque_limit", f32 * LG_MAX_DOF),
        ("cp_count", i32 * LG_MAX_LEGS), ("cp_link", (i32 * LG_MAX_CP) * LG_MAX_LEGS), ("cp_body", (i32 * LG_MAX_CP) * LG_MAX_LEGS),
        ("cp_pos", (f32 * 3) * LG_MAX_CP * LG_MAX_LEGS), ("cp_radius", (f32 * LG_MAX_CP) * LG_MAX_LEGS),
        ("cp_slide", (f32 * 3) * LG_MAX_CP * LG_MAX_LEGS),
        ("num_sc_pairs", i32), ("sc_pairs", (i32 * 4) * LG_MAX_SC_PAIRS),
        ("feet_indices", i32 * LG_MAX_LEGS),
        ("num_penalised", i32), ("penalised_contact_indices", i32 * LG_MAX_INDEX_LIST),
        ("num_termination", i32), ("termination_contact_indices", i32 * LG_MAX_INDEX_LIST),
    ]


class lg_terrain(C.Structure):
    _fields_ = [
        ("mesh_type", i32), ("rows", i32), ("cols", i32),
        ("horizontal_scale", f32), ("vertical_scale", f32), ("border_size", f32), ("static_friction", f32),
        ("height_samples", C.POINTER(C.c_int16)),
        ("num_levels", i32), ("num_types", i32),
        ("terrain_origins", C.POINTER(f32)),
        ("env_length", f32),
        ("collision_mesh", C.c_void_p),
        ("grid_vertices", C.POINTER(f32)),
    ]


class lg_config(C.Structure):
    _fields_ = [
        ("abi_version", i32), ("num_envs", i32), ("num_obs", i32), ("num_height_points", i32), ("num_extra_obs", i32),
        ("sim_dt", f32), ("decimation", i32), ("gravity", f32 * 3),
        ("control_type", i32), ("action_scale", f32),
        ("p_gains", f32 * LG_MAX_DOF), ("d_gains", f32 * LG_MAX_DOF), ("default_dof_pos", f32 * LG_MAX_DOF),
        ("clip_actions", f32), ("clip_observations", f32),
        ("actuator_net", f32 * LG_LSTM_NPARAM), ("actuator_in_scale", f32 * 2), ("actuator_out_scale", f32),
        ("obs_scale_lin_vel", f32), ("obs_scale_ang_vel", f32), ("obs_scale_dof_pos", f32), ("obs_scale_dof_vel", f32),
        ("obs_scale_height", f32),
        ("measure_heights", i32), ("add_noise", i32),
        ("noise_scale_vec", C.POINTER(f32)), ("height_points", C.POINTER(f32)),
        ("heading_command", i32), ("resampling_steps", i32),
        ("cmd_lin_vel_x", f32 * 2), ("cmd_lin_vel_y", f32 * 2), ("cmd_ang_vel_yaw", f32 * 2), ("cmd_heading", f32 * 2),
        ("command_curriculum", i32), ("max_curriculum", f32),
        ("push_robots", i32), ("push_interval", i32), ("max_push_vel_xy", f32),
        ("num_reward_terms", i32), ("reward_term_ids", i32 * LG_MAX_REWARD_TERMS),
        ("reward_scales", f32 * LG_MAX_REWARD_TERMS), ("only_positive_rewards", i32), ("reward_class", i32),
        ("tracking_sigma", f32), ("base_height_target", f32), ("max_contact_force", f32), ("soft_dof_vel_limit", f32),
        ("soft_torque_limit", f32),
        ("dof_pos_limits", (f32 * 2) * LG_MAX_DOF),
        ("max_episode_length", f32), ("max_episode_length_s", f32),
        ("curriculum", i32), ("custom_origins", i32), ("max_terrain_level", i32),
        ("reset_z_from_terrain", i32),
        ("terminate_on_flip", i32),
        ("base_init_state", f32 * 13),
        ("gait_enabled", i32), ("gait_period", f32), ("gait_swing_height", f32), ("gait_foot_phases", f32 * LG_MAX_LEGS),
        ("solver_iterations", i32), ("contact_offset", f32), ("max_depenetration_velocity", f32), ("erp", f32),
        ("cfm", f32), ("solver_type", i32), ("friction_model", i32), ("self_collisions", i32),
        ("seed", C.c_uint64), ("rng_mode", i32),
        ("async_num_dof_sets", i32), ("async_dof_sets", (i32 * 3) * 4), ("async_dof_nominal", f32 * LG_MAX_DOF), ("async_dof_weight", f32 * LG_MAX_DOF),
        ("async_weights", f32 * 3), ("async_foot_z_align", f32), ("keep_small_commands", i32), ("feet_air_time_ungated", i32), ("inject_sim_state", i32),
    ]


class lg_tile_spec(C.Structure):
    _fields_ = [("kind", i32), ("max_height", i32), ("clip_lo", i32), ("clip_hi", i32), ("step_width", i32), ("step_height", i32),
                ("num_steps", i32), ("noise_lo", i32), ("noise_step", i32), ("noise_levels", i32), ("noise_coarse", i32),
                ("rect_min", i32), ("rect_max", i32), ("rect_count", i32), ("platform", i32), ("seed", C.c_uint32)]


LG_TILE_FLAT, LG_TILE_PYRAMID_SLOPE, LG_TILE_PYRAMID_STAIRS, LG_TILE_DISCRETE_OBSTACLES = 0, 1, 2, 3
LG_TILE_STEPPING_STONES, LG_TILE_GAP, LG_TILE_PIT = 4, 5, 6


class lg_pose_params(C.Structure):
    _fields_ = [("ranges", (f32 * 2) * 4), ("resampling_steps", i32), ("scale_orientation", f32), ("scale_base_height", f32),
                ("scale_termination", f32), ("only_positive_rewards", i32), ("max_episode_length_s", f32), ("clip_observations", f32),
                ("num_heights", i32), ("num_proprio", i32)]


class lg_foottrack_params(C.Structure):
    _fields_ = [("dt", f32), ("gait_period", f32), ("swing_ema", f32), ("reward_sigma", f32), ("swing_height", f32), ("phase_offsets", f32 * 6),
                ("base_bounds", (f32 * 6) * 2), ("foot_mean", f32 * 18), ("foot_sigma", f32 * 18), ("base_interval", f32), ("base_max_vel", f32),
                ("foot_interval", f32), ("foot_max_vel", f32), ("scales", f32 * 5), ("scale_termination", f32), ("only_positive_rewards", i32),
                ("max_episode_length_s", f32), ("clip_observations", f32), ("num_bodies", i32), ("feet_indices", i32 * 6), ("add_noise", i32)]


class lg_foottrack_state(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("base_pos", "base_quat", "base_pos_shift", "base_quat_shift", "base_x_world", "base_y_world", "foot_pos", "gait_idx",
                                          "gait_phases", "last_contacts", "bw_cur", "bw_tgt", "bw_timer", "fw_cur", "fw_tgt", "fw_timer")]


class lg_depth_params(C.Structure):
    _fields_ = [("width", i32), ("height", i32), ("resized_width", i32), ("resized_height", i32), ("buffer_len", i32),
                ("near_clip", f32), ("far_clip", f32), ("position", f32 * 3), ("quat_offset", f32 * 4)]


def declare_product(lib):
    """Prototypes of liblgstep.so (include/lgstep.h)."""
    vp = C.c_void_p
    lib.lg_abi_sizes.argtypes = [C.POINTER(i32)]
    lib.lg_abi_sizes.restype = None
    lib.lg_arena_bytes.argtypes = [C.POINTER(lg_config), C.POINTER(lg_robot_model), C.POINTER(lg_terrain)]
    lib.lg_arena_bytes.restype = C.c_size_t
    lib.lg_create.argtypes = [C.POINTER(lg_config), C.POINTER(lg_robot_model), C.POINTER(lg_terrain), C.c_int, vp]
    lib.lg_create.restype = vp
    lib.lg_get_tensor.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(C.c_int64), C.POINTER(i32), C.POINTER(i32)]
    lib.lg_get_tensor.restype = C.c_int
    lib.lg_step.argtypes = [vp, vp, vp]
    lib.lg_step.restype = C.c_int
    lib.lg_step_physics.argtypes = [vp, vp, vp]
    lib.lg_step_physics.restype = C.c_int
    lib.lg_step_subset.argtypes = [vp, vp, vp, i32, i32, vp]
    lib.lg_step_subset.restype = C.c_int
    lib.lg_set_reward_terms.argtypes = [vp, i32, C.POINTER(i32), C.POINTER(f32), vp]
    lib.lg_set_reward_terms.restype = C.c_int
    lib.lg_set_async_gait.argtypes = [vp, C.POINTER(f32), f32, vp]
    lib.lg_set_async_gait.restype = C.c_int
    lib.lg_set_lattice_capsules.argtypes = [vp, i32]
    lib.lg_set_lattice_capsules.restype = C.c_int
    lib.lg_step_subset_physics.argtypes = [vp, vp, vp, i32, vp]
    lib.lg_step_subset_physics.restype = C.c_int
    lib.lg_post_physics_subset.argtypes = [vp, vp, i32, i32, vp]
    lib.lg_post_physics_subset.restype = C.c_int
    lib.lg_sync_main_to_rollout.argtypes = [vp, i32, f32, vp]
    lib.lg_sync_main_to_rollout.restype = C.c_int
    lib.lg_step_transition.argtypes = [vp, vp, vp, vp, f32, vp, vp, vp]
    lib.lg_step_transition.restype = C.c_int
    lib.lg_rollout_batch.argtypes = [vp, vp, i32, vp, i32, i32, f32, vp, vp]
    lib.lg_rollout_batch.restype = C.c_int
    lib.lg_compute_torques.argtypes = [vp, vp, vp]
    lib.lg_compute_torques.restype = C.c_int
    lib.lg_simulate.argtypes = [vp, vp]
    lib.lg_simulate.restype = C.c_int
    lib.lg_post_physics_step.argtypes = [vp, vp]
    lib.lg_post_physics_step.restype = C.c_int
    lib.lg_reset_idx.argtypes = [vp, vp, i32, i32, vp]
    lib.lg_reset_idx.restype = C.c_int
    lib.lg_set_state_indexed.argtypes = [vp, vp, vp, vp, i32, vp]
    lib.lg_set_state_indexed.restype = C.c_int
    lib.lg_gather_step_rows.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp]
    lib.lg_gather_step_rows.restype = C.c_int
    lib.lg_step_subset_rows.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp, vp, vp]
    lib.lg_step_subset_rows.restype = C.c_int
    lib.lg_step_rollout.argtypes = [vp, vp, vp, i32, vp, vp, vp, vp, vp]
    lib.lg_step_rollout.restype = C.c_int
    lib.lg_set_extra_termination.argtypes = [vp, vp]
    lib.lg_set_extra_termination.restype = C.c_int
    lib.lg_set_extra_obs.argtypes = [vp, vp]
    lib.lg_set_extra_obs.restype = C.c_int
    lib.lg_terrain_generate.argtypes = [C.POINTER(lg_tile_spec), i32, i32, i32, i32, i32, f32, f32, f32, f32, vp, vp, vp]
    lib.lg_terrain_generate.restype = C.c_int
    lib.lg_heightfield_to_trimesh.argtypes = [vp, i32, i32, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, vp, vp, vp]
    lib.lg_heightfield_to_trimesh.restype = C.c_int
    lib.lg_pose_layer_step.argtypes = [C.POINTER(lg_pose_params), i32, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.lg_pose_layer_step.restype = C.c_int
    lib.lg_foottrack_stray.argtypes = [i32, vp, vp, vp, vp, vp]
    lib.lg_foottrack_stray.restype = C.c_int
    lib.lg_foottrack_layer_step.argtypes = [C.POINTER(lg_foottrack_params), C.POINTER(lg_foottrack_state), i32, i32] + [vp] * 8 + [i32] + [vp] * 10
    lib.lg_foottrack_layer_step.restype = C.c_int
    lib.lg_mesh_create.argtypes = [C.POINTER(f32), C.c_int64, C.POINTER(i32), C.c_int64, C.c_int]
    lib.lg_mesh_create.restype = vp
    lib.lg_mesh_destroy.argtypes = [vp]
    lib.lg_mesh_destroy.restype = None
    lib.lg_mesh_info.argtypes = [vp, C.POINTER(C.c_int64)]
    lib.lg_mesh_info.restype = C.c_int
    lib.lg_mesh_ray_lattice.argtypes = [vp, C.POINTER(C.c_int32)]
    lib.lg_mesh_ray_lattice.restype = C.c_int
    lib.lg_mesh_contact_lattice.argtypes = [vp, C.POINTER(C.c_int32)]
    lib.lg_mesh_contact_lattice.restype = C.c_int
    lib.lg_mesh_last_error.argtypes = [vp]
    lib.lg_mesh_last_error.restype = C.c_char_p
    lib.lg_raycast_mesh.argtypes = [vp, vp, vp, C.c_int64, f32, vp, vp, vp]
    lib.lg_raycast_mesh.restype = C.c_int
    lib.lg_mesh_query_sdf.argtypes = [vp, vp, C.c_int64, f32, vp, vp, vp]
    lib.lg_mesh_query_sdf.restype = C.c_int
    lib.lg_raycaster_update.argtypes = [vp, vp, vp, vp, i32, i32, f32, i32, vp, vp, vp, vp]
    lib.lg_raycaster_update.restype = C.c_int
    lib.lg_raycaster_update_subset.argtypes = [vp, vp, vp, vp, i32, f32, i32, vp, i32, vp, vp, vp, i32, vp]
    lib.lg_raycaster_update_subset.restype = C.c_int
    lib.lg_sdf_bodies_update.argtypes = [vp, vp, i32, vp, vp, i32, vp, i32, f32, vp, i32, vp, vp, vp]
    lib.lg_sdf_bodies_update.restype = C.c_int
    lib.lg_depth_camera_update.argtypes = [vp, C.POINTER(lg_depth_params), vp, vp, vp, i32, vp, vp, vp, vp, vp]
    lib.lg_depth_camera_update.restype = C.c_int
    lib.lg_profile_begin.argtypes = [vp, i32, i32]
    lib.lg_profile_begin.restype = C.c_int
    lib.lg_profile_end.argtypes = [vp, C.POINTER(f32), C.POINTER(i32)]
    lib.lg_profile_end.restype = C.c_int
    lib.lg_last_error.argtypes = [vp]
    lib.lg_last_error.restype = C.c_char_p
    lib.lg_destroy.argtypes = [vp]
    lib.lg_destroy.restype = None
    return lib


class lg_rollout(C.Structure):
    """include/lgpolicy.h: device pointers to the (T, n, .) rows of one collected rollout."""
    _fields_ = [(k, C.c_void_p) for k in ("observations", "actions", "rewards", "dones", "values", "actions_log_prob", "mu", "sigma",
                                          "last_values", "returns", "advantages")]


class lg_rollout_hidden(C.Structure):
    """include/lgpolicy.h: device pointers to the (T, L, n, H) hidden-state rows of one collected rollout (state before each step's act)."""
    _fields_ = [(k, C.c_void_p) for k in ("h_a", "c_a", "h_c", "c_c")]


class lg_distill_rollout(C.Structure):
    """include/lgpolicy.h: device pointers to the (T, n, .) rows of one collected distillation rollout (+ the student's row after the last step)."""
    _fields_ = [(k, C.c_void_p) for k in ("observations", "privileged_observations", "actions", "privileged_actions", "rewards", "dones",
                                          "last_observations")]


class lg_obs_history(C.Structure):
    """include/lgpolicy.h: the observation-history layer between the env's row and the student."""
    _fields_ = [("history", C.c_void_p), ("H", i32), ("W", i32), ("noise_scale", C.c_void_p), ("clip", f32), ("noise_seed", C.c_uint64),
                ("inject_u", C.c_void_p)]


def declare_policy_wide(lib):
    """Prototype of include/lgpolicy_wide.h: `lg_mlp_create` for an input row of up to MLP_MAX_INPUT columns."""
    lib.lg_mlp_create_wide.argtypes = [i32, C.POINTER(i32), C.POINTER(C.POINTER(f32)), C.POINTER(C.POINTER(f32)), i32, C.c_int]
    lib.lg_mlp_create_wide.restype = C.c_void_p
    # include/lgpolicy_wide_memory.h: `lg_rnn_create` for an input row of up to RNN_MAX_INPUT columns, and the host tiling of its two images
    fpp = C.POINTER(C.POINTER(f32))
    lib.lg_rnn_create_wide.argtypes = [i32, i32, i32, i32, fpp, fpp, fpp, fpp, C.c_int]
    lib.lg_rnn_create_wide.restype = C.c_void_p
    lib.lg_rnn_tile_weights_wide.argtypes = [i32, i32, i32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
    lib.lg_rnn_tile_weights_wide.restype = C.c_int64
    return lib


def declare_policy(lib):
    """Prototypes of the rollout-collection entry points (include/lgpolicy.h), same library."""
    vp = C.c_void_p
    lib.lg_mlp_create.argtypes = [i32, C.POINTER(i32), C.POINTER(C.POINTER(f32)), C.POINTER(C.POINTER(f32)), i32, C.c_int]
    lib.lg_mlp_create.restype = vp
    lib.lg_mlp_destroy.argtypes = [vp]
    lib.lg_mlp_destroy.restype = None
    lib.lg_mlp_last_error.argtypes = [vp]
    lib.lg_mlp_last_error.restype = C.c_char_p
    lib.lg_mlp_forward.argtypes = [vp, vp, C.c_int64, vp, vp]
    lib.lg_mlp_forward.restype = C.c_int
    lib.lg_policy_act.argtypes = [vp, vp, vp, vp, C.c_int64, vp, C.c_uint64, C.c_uint64, i32, vp, vp, vp, vp, vp]
    lib.lg_policy_act.restype = C.c_int
    lib.lg_compute_returns.argtypes = [vp, vp, vp, vp, i32, C.c_int64, f32, f32, i32, vp, vp, vp]
    lib.lg_compute_returns.restype = C.c_int
    lib.lg_collect_rollout.argtypes = [vp, vp, vp, vp, C.c_uint64, C.c_uint64, i32, f32, f32, i32, C.POINTER(lg_rollout), vp]
    lib.lg_collect_rollout.restype = C.c_int
    lib.lg_plan_from_nodes.argtypes = [vp, vp, C.c_int64, i32, i32, i32, vp, vp]
    lib.lg_plan_from_nodes.restype = C.c_int
    lib.lg_mppi_update.argtypes = [vp, vp, i32, i32, i32, i32, i32, f32, vp, vp, vp]
    lib.lg_mppi_update.restype = C.c_int
    u64 = C.c_uint64
    lib.lg_mppi_sample_plans.argtypes = [vp, vp, f32, vp, i32, i32, i32, i32, i32, u64, u64, vp, vp, vp]
    lib.lg_mppi_sample_plans.restype = C.c_int
    lib.lg_planner_diffuse.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, f32, f32, u64, u64, vp, i32, f32, vp, vp, vp, vp, vp]
    lib.lg_planner_diffuse.restype = C.c_int
    fpp = C.POINTER(C.POINTER(f32))
    lib.lg_rnn_create.argtypes = [i32, i32, i32, i32, fpp, fpp, fpp, fpp, C.c_int]
    lib.lg_rnn_create.restype = vp
    lib.lg_rnn_destroy.argtypes = [vp]
    lib.lg_rnn_destroy.restype = None
    lib.lg_rnn_tile_weights.argtypes = [i32, i32, i32, vp, vp, vp]
    lib.lg_rnn_tile_weights.restype = C.c_int64
    lib.lg_rnn_step.argtypes = [vp, vp, C.c_int64, vp, vp, vp, vp, vp]
    lib.lg_rnn_step.restype = C.c_int
    lib.lg_rnn_reset_rows.argtypes = [vp, vp, vp, vp, C.c_int64, vp]
    lib.lg_rnn_reset_rows.restype = C.c_int
    lib.lg_policy_act_recurrent.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int64, vp, u64, u64, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.lg_policy_act_recurrent.restype = C.c_int
    lib.lg_collect_rollout_recurrent.argtypes = [vp, vp, vp, vp, vp, vp, u64, u64, i32, f32, f32, i32, C.POINTER(lg_rollout), C.POINTER(lg_rollout_hidden),
                                                 vp, vp, vp, vp, vp]
    lib.lg_collect_rollout_recurrent.restype = C.c_int
    lib.lg_obs_history_step.argtypes = [vp, C.c_int64, i32, i32, vp, C.c_int64, vp, vp, vp, u64, u64, f32, vp, vp]
    lib.lg_obs_history_step.restype = C.c_int
    lib.lg_distill_act.argtypes = [vp, vp, vp, vp, C.c_int64, vp, u64, u64, i32, vp, vp, vp, vp]
    lib.lg_distill_act.restype = C.c_int
    lib.lg_distill_act_recurrent.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int64, vp, u64, u64, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.lg_distill_act_recurrent.restype = C.c_int
    lib.lg_collect_distillation.argtypes = [vp, vp, vp, vp, u64, u64, i32, C.POINTER(lg_obs_history), C.POINTER(lg_distill_rollout), vp]
    lib.lg_collect_distillation.restype = C.c_int
    lib.lg_collect_distillation_recurrent.argtypes = [vp, vp, vp, vp, vp, vp, u64, u64, i32, C.POINTER(lg_obs_history), C.POINTER(lg_distill_rollout)] + [vp] * 9
    lib.lg_collect_distillation_recurrent.restype = C.c_int
    lib.lg_conv_encoder_create.argtypes = [i32, i32, i32, i32, fpp, fpp, C.c_int]
    lib.lg_conv_encoder_create.restype = vp
    lib.lg_conv_encoder_destroy.argtypes = [vp]
    lib.lg_conv_encoder_destroy.restype = None
    lib.lg_conv_tile_weights.argtypes = [i32, i32, i32, i32, vp, vp]
    lib.lg_conv_tile_weights.restype = C.c_int64
    lib.lg_conv_encoder_forward.argtypes = [vp, vp, C.c_int64, C.c_int64, vp, vp]
    lib.lg_conv_encoder_forward.restype = C.c_int
    lib.lg_conv_encoder_stage_shape.argtypes = [vp, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    lib.lg_conv_encoder_stage_shape.restype = C.c_int64
    lib.lg_conv_encoder_forward_stages.argtypes = [vp, vp, C.c_int64, C.c_int64, i32, vp, vp]
    lib.lg_conv_encoder_forward_stages.restype = C.c_int
    lib.lg_mlp_set_output_activation.argtypes = [vp, i32]
    lib.lg_mlp_set_output_activation.restype = C.c_int
    lib.lg_estimator_step.argtypes = [vp, vp, vp, vp, vp, C.c_int64, vp, C.c_int64, vp, vp, vp, vp, vp]
    lib.lg_estimator_step.restype = C.c_int
    lib.lg_conv_encoder_create_precision.argtypes = [i32, i32, i32, i32, fpp, fpp, C.c_int, i32]
    lib.lg_conv_encoder_create_precision.restype = vp
    lib.lg_conv_encoder_precision.argtypes = [vp]
    lib.lg_conv_encoder_precision.restype = i32
    lib.lg_conv_tile_weights_bf16.argtypes = [i32, i32, i32, i32, vp, vp]
    lib.lg_conv_tile_weights_bf16.restype = C.c_int64
    return lib


class lg_ppo_rows(C.Structure):
    """include/lgtrain.h: device pointers to the flattened (R, .) rows of a rollout."""
    _fields_ = [(k, C.c_void_p) for k in ("observations", "critic_observations", "actions", "values", "returns", "advantages", "actions_log_prob",
                                          "mu", "sigma")]


class lg_ppo_hyper(C.Structure):
    """include/lgtrain.h: the hyper-parameters of one optimiser step."""
    _fields_ = [("clip_param", f32), ("value_loss_coef", f32), ("entropy_coef", f32), ("use_clipped_value_loss", i32), ("max_grad_norm", f32),
                ("schedule", i32), ("desired_kl", C.c_double)]


class lg_ppo_stats(C.Structure):
    """include/lgtrain.h: what an update reports (float64, device memory)."""
    _fields_ = [(k, C.c_double) for k in ("value_function", "surrogate", "entropy", "kl", "learning_rate")]


def _declare_trainer_group(lib, prefix, carry=False, workspace=False, step_losses=False):
    """The prototypes every native trainer exports under its own prefix: the parameter count, the checkpoint calls and the learning rate; optionally the
    workspace size, the step losses of the last update and the carried memory state."""
    vp, i64 = C.c_void_p, C.c_int64

    def declare(name, argtypes, restype=C.c_int):
        fn = getattr(lib, "%s_%s" % (prefix, name))
        fn.argtypes, fn.restype = argtypes, restype

    declare("parameter_count", [vp], i64)
    declare("get_parameters", [vp, vp, vp])
    declare("get_state", [vp, vp, vp, vp, C.POINTER(i64), C.POINTER(C.c_double), vp])
    declare("set_state", [vp, vp, vp, vp, i64, C.c_double, vp])
    declare("set_learning_rate", [vp, C.c_double, vp])
    if workspace:
        declare("workspace_bytes", [vp], i64)
    if step_losses:
        declare("step_losses", [vp, vp, i64, vp])
    if carry:
        declare("get_carry", [vp, vp, vp, i64, i32, vp], i64)
        declare("set_carry", [vp, vp, vp, i64, vp])
        declare("reset_carry", [vp, vp])


def declare_train(lib):
    """Prototypes of the training entry points (include/lgtrain.h), same library."""
    vp, fpp = C.c_void_p, C.POINTER(C.POINTER(f32))
    lib.lg_ppo_create.argtypes = [vp, vp, fpp, fpp, fpp, fpp, vp, i32, C.c_double, C.c_int64, vp]
    lib.lg_ppo_create.restype = vp
    lib.lg_ppo_destroy.argtypes = [vp]
    lib.lg_ppo_destroy.restype = None
    lib.lg_ppo_minibatch.argtypes = [vp, C.POINTER(lg_ppo_rows), vp, C.c_int64, C.POINTER(lg_ppo_hyper), vp]
    lib.lg_ppo_minibatch.restype = C.c_int
    lib.lg_ppo_update.argtypes = [vp, C.POINTER(lg_ppo_rows), C.c_int64, vp, i32, i32, C.POINTER(lg_ppo_hyper), vp, vp]
    lib.lg_ppo_update.restype = C.c_int
    lib.lg_ppo_gradients.argtypes = [vp, vp, vp, vp, vp]
    lib.lg_ppo_gradients.restype = C.c_int
    lib.lg_ppo_forward_outputs.argtypes = [vp, vp, vp, vp]
    lib.lg_ppo_forward_outputs.restype = C.c_int
    lib.lg_ppo_wgrad_slab_rows.argtypes = []
    lib.lg_ppo_wgrad_slab_rows.restype = i32
    _declare_trainer_group(lib, "lg_ppo")
    return lib


class lg_ppo_sym_tables(C.Structure):
    """include/lgtrain_symmetry.h: HOST signed-permutation tables, (num_blocks, width) each."""
    _fields_ = ([(k, i32) for k in ("num_blocks", "observation_width", "critic_observation_width", "action_width")] +
                [(k, C.c_void_p) for k in ("observation_perm", "observation_sign", "critic_observation_perm", "critic_observation_sign", "action_perm",
                                           "action_sign")])


class lg_ppo_sym_config(C.Structure):
    """include/lgtrain_symmetry.h: the symmetry option of PPO."""
    _fields_ = [("use_data_augmentation", i32), ("use_mirror_loss", i32), ("mirror_loss_coeff", f32)]


class lg_ppo_sym_stats(C.Structure):
    """include/lgtrain_symmetry.h: lg_ppo_stats and the symmetry mean (float64, device memory)."""
    _fields_ = [(k, C.c_double) for k in ("value_function", "surrogate", "entropy", "kl", "learning_rate", "symmetry")]


SYMMETRY_MAX_BLOCKS = 4          # LG_PPO_SYM_MAX_BLOCKS


def declare_train_symmetry(lib):
    """Prototypes of the symmetric PPO trainer (include/lgtrain_symmetry.h), same library."""
    vp, fpp, i64 = C.c_void_p, C.POINTER(C.POINTER(f32)), C.c_int64
    lib.lg_ppo_sym_create.argtypes = [vp, vp, fpp, fpp, fpp, fpp, vp, i32, C.c_double, i64, vp, C.POINTER(lg_ppo_sym_tables), C.POINTER(lg_ppo_sym_config)]
    lib.lg_ppo_sym_create.restype = vp
    lib.lg_ppo_sym_destroy.argtypes = [vp]
    lib.lg_ppo_sym_destroy.restype = None
    lib.lg_ppo_sym_minibatch.argtypes = [vp, C.POINTER(lg_ppo_rows), vp, i64, C.POINTER(lg_ppo_hyper), vp]
    lib.lg_ppo_sym_minibatch.restype = C.c_int
    lib.lg_ppo_sym_update.argtypes = [vp, C.POINTER(lg_ppo_rows), i64, vp, i32, i32, C.POINTER(lg_ppo_hyper), vp, vp]
    lib.lg_ppo_sym_update.restype = C.c_int
    lib.lg_ppo_sym_gradients.argtypes = [vp, vp, vp, vp, vp, vp]
    lib.lg_ppo_sym_gradients.restype = C.c_int
    lib.lg_ppo_sym_forward_outputs.argtypes = [vp, vp, vp, vp]
    lib.lg_ppo_sym_forward_outputs.restype = C.c_int
    _declare_trainer_group(lib, "lg_ppo_sym")
    return lib


class lg_ppo_recurrent_params(C.Structure):
    """include/lgtrain_recurrent.h: HOST parameters of an ActorCriticRecurrent in torch's layout, and the shapes they were taken from."""
    _fields_ = ([(k, i32) for k in ("rnn_type", "num_layers", "input_a", "hidden_a", "input_c", "hidden_c")] +
                [(k, C.POINTER(C.POINTER(f32))) for k in ("mem_a_w_ih", "mem_a_w_hh", "mem_a_b_ih", "mem_a_b_hh", "mem_c_w_ih", "mem_c_w_hh", "mem_c_b_ih",
                                                         "mem_c_b_hh", "actor_weights", "actor_biases", "critic_weights", "critic_biases")] +
                [("std", C.c_void_p)])


def declare_train_recurrent(lib):
    """Prototypes of the recurrent PPO trainer (include/lgtrain_recurrent.h), same library."""
    vp, i64 = C.c_void_p, C.c_int64
    rows, hid, hyp = C.POINTER(lg_ppo_rows), C.POINTER(lg_rollout_hidden), C.POINTER(lg_ppo_hyper)
    lib.lg_ppo_recurrent_create.argtypes = [vp, vp, vp, vp, C.POINTER(lg_ppo_recurrent_params), i32, C.c_double, i64, vp]
    lib.lg_ppo_recurrent_create.restype = vp
    lib.lg_ppo_recurrent_destroy.argtypes = [vp]
    lib.lg_ppo_recurrent_destroy.restype = None
    lib.lg_ppo_recurrent_minibatch.argtypes = [vp, rows, hid, vp, i32, i64, i64, i64, hyp, vp]
    lib.lg_ppo_recurrent_minibatch.restype = C.c_int
    lib.lg_ppo_recurrent_update.argtypes = [vp, rows, hid, vp, i32, i64, i32, i32, hyp, vp, vp]
    lib.lg_ppo_recurrent_update.restype = C.c_int
    lib.lg_ppo_recurrent_gradients.argtypes = [vp, vp, vp, vp, vp]
    lib.lg_ppo_recurrent_gradients.restype = C.c_int
    lib.lg_ppo_recurrent_forward_outputs.argtypes = [vp, vp, vp, vp]
    lib.lg_ppo_recurrent_forward_outputs.restype = C.c_int
    lib.lg_ppo_recurrent_get_images.argtypes = [vp, i32, i32, vp, vp, vp]
    lib.lg_ppo_recurrent_get_images.restype = C.c_int
    _declare_trainer_group(lib, "lg_ppo_recurrent", workspace=True)
    return lib


class lg_distill_train_hyper(C.Structure):
    """include/lgdistill.h: the loss and the clip of one optimiser step (max_grad_norm <= 0: no clip)."""
    _fields_ = [("loss_type", i32), ("max_grad_norm", f32)]


class lg_distill_train_stats(C.Structure):
    """include/lgdistill.h: what an update reports (float64, device memory)."""
    _fields_ = [(k, C.c_double) for k in ("behavior", "optimizer_steps", "grad_norm")]


def declare_distill_train(lib):
    """Prototypes of the distillation trainer (include/lgdistill.h), same library."""
    vp, fpp, i64 = C.c_void_p, C.POINTER(C.POINTER(f32)), C.c_int64
    hp = C.POINTER(lg_distill_train_hyper)
    lib.lg_distill_train_create.argtypes = [vp, fpp, fpp, C.c_double, i64]
    lib.lg_distill_train_create.restype = vp
    lib.lg_distill_train_destroy.argtypes = [vp]
    lib.lg_distill_train_destroy.restype = None
    lib.lg_distill_train_group.argtypes = [vp, vp, vp, i64, i64, i64, i64, hp, vp]
    lib.lg_distill_train_group.restype = C.c_int
    lib.lg_distill_train_update.argtypes = [vp, vp, vp, i64, i64, i32, i32, hp, vp, vp]
    lib.lg_distill_train_update.restype = C.c_int
    lib.lg_distill_train_gradients.argtypes = [vp, vp, vp, vp, i64, vp]
    lib.lg_distill_train_gradients.restype = C.c_int
    lib.lg_distill_train_forward_outputs.argtypes = [vp, vp, vp]
    lib.lg_distill_train_forward_outputs.restype = C.c_int
    _declare_trainer_group(lib, "lg_distill_train", step_losses=True)
    return lib


DISTILL_LOSSES = {"mse": 0, "huber": 1}          # enum lg_distill_loss


class lg_distill_rtrain_params(C.Structure):
    """include/lgdistill_recurrent.h: HOST pointers to the trained tensors (student.*, memory_s.*) in torch's layout."""
    _fields_ = [(k, C.POINTER(C.POINTER(f32))) for k in ("student_weights", "student_biases", "memory_w_ih", "memory_w_hh", "memory_b_ih", "memory_b_hh")]


class lg_distill_rtrain_stats(C.Structure):
    """include/lgdistill_recurrent.h: what an update reports (float64, device memory)."""
    _fields_ = [(k, C.c_double) for k in ("behavior", "optimizer_steps", "grad_norm", "memory_grad_norm")]


def declare_distill_rtrain(lib):
    """Prototypes of the recurrent student's distillation trainer (include/lgdistill_recurrent.h), same library."""
    vp, i64 = C.c_void_p, C.c_int64
    hp = C.POINTER(lg_distill_train_hyper)
    lib.lg_distill_rtrain_create.argtypes = [vp, vp, C.POINTER(lg_distill_rtrain_params), C.c_double, i64]
    lib.lg_distill_rtrain_create.restype = vp
    lib.lg_distill_rtrain_destroy.argtypes = [vp]
    lib.lg_distill_rtrain_destroy.restype = None
    lib.lg_distill_rtrain_group.argtypes = [vp, vp, vp, vp, i64, i64, i64, i64, i32, hp, vp]
    lib.lg_distill_rtrain_group.restype = C.c_int
    lib.lg_distill_rtrain_update.argtypes = [vp, vp, vp, vp, i64, i64, i32, i32, hp, vp, vp]
    lib.lg_distill_rtrain_update.restype = C.c_int
    lib.lg_distill_rtrain_student_parameter_count.argtypes = [vp]
    lib.lg_distill_rtrain_student_parameter_count.restype = i64
    lib.lg_distill_rtrain_gradients.argtypes = [vp, vp, vp, vp, i64, vp]
    lib.lg_distill_rtrain_gradients.restype = C.c_int
    lib.lg_distill_rtrain_forward_outputs.argtypes = [vp, vp, vp]
    lib.lg_distill_rtrain_forward_outputs.restype = C.c_int
    _declare_trainer_group(lib, "lg_distill_rtrain", carry=True, workspace=True, step_losses=True)
    return lib


class lg_estimator_train_hyper(C.Structure):
    """include/lgestimator_train.h: the loss, the clip (max_grad_norm <= 0: no clip) and whether the rows' dones reset the memory."""
    _fields_ = [("loss_type", i32), ("max_grad_norm", f32), ("use_dones", i32)]


class lg_estimator_train_params(C.Structure):
    """include/lgestimator_train.h: HOST pointers to the module's tensors in torch's layout."""
    _fields_ = [(k, C.POINTER(f32) if k.startswith("combine") else C.POINTER(C.POINTER(f32)))
                for k in ("encoder_weights", "encoder_biases", "combine_weight", "combine_bias", "memory_w_ih", "memory_w_hh", "memory_b_ih", "memory_b_hh",
                          "decoder_weights", "decoder_biases")]


class lg_estimator_train_stats(C.Structure):
    """include/lgestimator_train.h: what an update reports (float64, device memory)."""
    _fields_ = [(k, C.c_double) for k in ("estimation", "optimizer_steps", "grad_norm")]


def declare_estimator_train(lib):
    """Prototypes of the terrain estimator's trainer (include/lgestimator_train.h), same library."""
    vp, i64 = C.c_void_p, C.c_int64
    hp = C.POINTER(lg_estimator_train_hyper)
    lib.lg_estimator_train_create.argtypes = [vp, vp, vp, vp, C.POINTER(lg_estimator_train_params), C.c_double, i64]
    lib.lg_estimator_train_create.restype = vp
    lib.lg_estimator_train_destroy.argtypes = [vp]
    lib.lg_estimator_train_destroy.restype = None
    lib.lg_estimator_train_group.argtypes = [vp, vp, vp, vp, vp, i64, i64, i64, i64, i32, hp, vp]
    lib.lg_estimator_train_group.restype = C.c_int
    lib.lg_estimator_train_update.argtypes = [vp, vp, vp, vp, vp, i64, i64, i32, i32, hp, vp, vp]
    lib.lg_estimator_train_update.restype = C.c_int
    lib.lg_estimator_train_wgrad_slab_rows.argtypes = []
    lib.lg_estimator_train_wgrad_slab_rows.restype = i32
    lib.lg_estimator_train_gradients.argtypes = [vp, vp, vp, vp, i64, vp]
    lib.lg_estimator_train_gradients.restype = C.c_int
    lib.lg_estimator_train_forward_outputs.argtypes = [vp, vp, vp]
    lib.lg_estimator_train_forward_outputs.restype = C.c_int
    _declare_trainer_group(lib, "lg_estimator_train", carry=True, workspace=True, step_losses=True)
    return lib


def declare_estimator_train_bf16(lib):
    """Prototypes of the bf16-encoder trainer's own entry points (include/lgestimator_train_bf16.h), same library; the handle it creates takes every
    call of `declare_estimator_train`."""
    vp, i64 = C.c_void_p, C.c_int64
    lib.lg_estimator_bf16train_create.argtypes = [vp, vp, vp, vp, C.POINTER(lg_estimator_train_params), C.c_double, i64]
    lib.lg_estimator_bf16train_create.restype = vp
    lib.lg_estimator_bf16train_wgrad_slab_rows.argtypes = []
    lib.lg_estimator_bf16train_wgrad_slab_rows.restype = i32
    lib.lg_estimator_bf16train_saved_stage.argtypes = [vp, i32, vp, i64, vp]
    lib.lg_estimator_bf16train_saved_stage.restype = C.c_int
    lib.lg_estimator_bf16train_backward_stage.argtypes = [vp, i32, vp, i64, vp, vp, vp]
    lib.lg_estimator_bf16train_backward_stage.restype = C.c_int
    return lib


ESTIMATOR_LOSSES = {"mse": 0, "huber": 1, "l1": 2}          # enum lg_estimator_loss
# enum lg_estimator_bf16_stage
ESTIMATOR_BF16_STAGES = {"pool_backward": 0, "dgrad_conv4": 1, "dgrad_conv3": 2, "dgrad_conv2": 3, "wgrad_conv4": 4, "wgrad_conv3": 5, "wgrad_conv2": 6, "wgrad_conv1": 7,
                         "linear2": 8, "linear1": 9}
ENCODER_TRAININGS = ("fp32", "bf16")          # NativeEstimatorDistillation(encoder_training=...)

NOISE_STD_TYPES = {"scalar": 0, "log": 1}          # enum lg_noise_std_type
LR_SCHEDULES = {"fixed": 0, "adaptive": 1}          # enum lg_lr_schedule

LG_PREC_F32, LG_PREC_BF16 = 0, 1          # the encoder's precision modes (include/lgpolicy.h)
ENCODER_PRECISIONS = {"fp32": LG_PREC_F32, "bf16": LG_PREC_BF16}
ENCODER_MAX_SIDE, ENCODER_MIN_SIDE, ENCODER_MAX_OUT = 128, 8, 512          # limits of lg_conv_encoder_create
MLP_MAX_WIDTH = 512          # widest layer of an lg_mlp, inputs included: MLP_MAXW of csrc/lg_policy.hip, held to it by tests/test_estimator_abi.py
MLP_MAX_INPUT = 2048         # widest input row of lg_mlp_create_wide: LG_MLP_MAX_INPUT of include/lgpolicy_wide.h (the other widths stay within MLP_MAX_WIDTH)
RNN_MAX_WIDTH = 512          # widest input of lg_rnn_create, and the hidden width's bound
RNN_MAX_INPUT = 2048         # widest input row of lg_rnn_create_wide: LG_RNN_MAX_INPUT of include/lgpolicy_wide_memory.h
RNN_TYPES = {"lstm": 0, "gru": 1}          # enum lg_rnn_type
ACTIVATIONS = {"elu": 0, "relu": 1, "tanh": 2, "lrelu": 3, "selu": 4}


class lg_runner_episode(C.Structure):
    """include/lgrunner.h: device pointers of the runner's episode bookkeeping over one collection."""
    _fields_ = [(k, C.c_void_p) for k in ("raw_rewards", "extras", "cur_reward_sum", "cur_episode_length", "ep_return", "ep_length")]


class lg_runner_hooks(C.Structure):
    """include/lgrunner.h: the two optional hooks of lg_runner_collect."""
    _fields_ = [("normalizer", C.c_void_p), ("training", i32), ("episode", C.POINTER(lg_runner_episode))]


def declare_runner(lib):
    """Prototypes of the runner's device pieces (include/lgrunner.h), same library."""
    vp, i64, u64 = C.c_void_p, C.c_int64, C.c_uint64
    lib.lg_obsnorm_create.argtypes = [i32, f32, i64, C.c_int]
    lib.lg_obsnorm_create.restype = vp
    lib.lg_obsnorm_destroy.argtypes = [vp]
    lib.lg_obsnorm_destroy.restype = None
    lib.lg_obsnorm_get_state.argtypes = [vp, vp, vp, vp, C.POINTER(i64), vp]
    lib.lg_obsnorm_get_state.restype = C.c_int
    lib.lg_obsnorm_set_state.argtypes = [vp, vp, vp, vp, i64, vp]
    lib.lg_obsnorm_set_state.restype = C.c_int
    lib.lg_obsnorm_step.argtypes = [vp, vp, i64, i64, i32, vp, vp]
    lib.lg_obsnorm_step.restype = C.c_int
    lib.lg_obsnorm_inverse.argtypes = [vp, vp, i64, i64, vp, vp]
    lib.lg_obsnorm_inverse.restype = C.c_int
    lib.lg_obsnorm_carried.argtypes = [vp, vp, i64, vp]
    lib.lg_obsnorm_carried.restype = C.c_int
    lib.lg_obsnorm_forget_carried.argtypes = [vp]
    lib.lg_obsnorm_forget_carried.restype = C.c_int
    lib.lg_runner_collect.argtypes = [vp, vp, vp, vp, vp, vp, u64, u64, i32, f32, f32, i32, C.POINTER(lg_rollout), C.POINTER(lg_rollout_hidden),
                                      vp, vp, vp, vp, C.POINTER(lg_runner_hooks), vp]
    lib.lg_runner_collect.restype = C.c_int
    lib.lg_runner_episode_track.argtypes = [vp, vp, i32, i64, vp, vp, vp, vp, vp]
    lib.lg_runner_episode_track.restype = C.c_int
    return lib


class lg_runner_privileged(C.Structure):
    """include/lgrunner_privileged.h: what lg_runner_collect_privileged takes beyond lg_runner_collect."""
    _fields_ = [("history", C.POINTER(lg_obs_history)), ("critic_normalizer", C.c_void_p), ("privileged_observations", C.c_void_p),
                ("last_observations", C.c_void_p)]


def declare_runner_privileged(lib):
    """Prototypes of the collection with privileged critic observations (include/lgrunner_privileged.h), same library."""
    vp, i64, u64 = C.c_void_p, C.c_int64, C.c_uint64
    lib.lg_obsnorm_step_pair.argtypes = [vp, vp, i64, vp, vp, vp, i64, vp, i64, i32, vp]
    lib.lg_obsnorm_step_pair.restype = C.c_int
    lib.lg_runner_collect_privileged.argtypes = [vp, vp, vp, vp, vp, vp, u64, u64, i32, f32, f32, i32, C.POINTER(lg_rollout), C.POINTER(lg_rollout_hidden),
                                                 vp, vp, vp, vp, C.POINTER(lg_runner_hooks), C.POINTER(lg_runner_privileged), vp]
    lib.lg_runner_collect_privileged.restype = C.c_int
    return lib


class lg_runner_distill(C.Structure):
    """include/lgrunner_distill.h: the hooks of lg_runner_collect_distillation(_recurrent)."""
    _fields_ = [("student_normalizer", C.c_void_p), ("teacher_normalizer", C.c_void_p), ("training", i32), ("episode", C.POINTER(lg_runner_episode))]


def declare_runner_distill(lib):
    """Prototypes of the runner's distillation collection (include/lgrunner_distill.h), same library."""
    vp, u64 = C.c_void_p, C.c_uint64
    lib.lg_runner_collect_distillation.argtypes = [vp, vp, vp, vp, u64, u64, i32, C.POINTER(lg_obs_history), C.POINTER(lg_distill_rollout),
                                                   C.POINTER(lg_runner_distill), vp]
    lib.lg_runner_collect_distillation.restype = C.c_int
    lib.lg_runner_collect_distillation_recurrent.argtypes = [vp, vp, vp, vp, vp, vp, u64, u64, i32, C.POINTER(lg_obs_history), C.POINTER(lg_distill_rollout)] + \
        [vp] * 8 + [C.POINTER(lg_runner_distill), vp]
    lib.lg_runner_collect_distillation_recurrent.restype = C.c_int
    return lib


class lg_sensor_raycaster(C.Structure):
    """include/lgsensors.h: the ray caster's parts of a sensor rig (device pointers to the Python object's own tensors)."""
    _fields_ = [("ray_origins", C.c_void_p), ("ray_dirs", C.c_void_p), ("num_rays", i32), ("max_distance", f32), ("attach_yaw_only", i32),
                ("ray_hits", C.c_void_p), ("hits_found", C.c_void_p), ("raycast_distances", C.c_void_p), ("distance_stride", i32)]


class lg_sensor_camera(C.Structure):
    """include/lgsensors.h: the depth camera's parts of a sensor rig."""
    _fields_ = [("params", lg_depth_params), ("ray_dirs", C.c_void_p), ("camera_pos", C.c_void_p), ("camera_rot", C.c_void_p),
                ("depth_buffer", C.c_void_p), ("update_interval", i32), ("counter", C.c_int64)]


class lg_estimation_out(C.Structure):
    """include/lgsensors.h: device pointers to the (T, n, .) rows of one estimation collection."""
    _fields_ = [(k, C.c_void_p) for k in ("depth_images", "proprio_data", "raycast_targets", "dones", "predictions")]


class lg_estimation_nets(C.Structure):
    """include/lgsensors.h: the four stages of `lg_estimator_step` and the memory's live state."""
    _fields_ = [(k, C.c_void_p) for k in ("encoder", "combine", "memory", "decoder", "h", "c")]


def declare_sensors(lib):
    """Prototypes of the sensors inside the one-call collectors (include/lgsensors.h), same library."""
    vp, i64, u64 = C.c_void_p, C.c_int64, C.c_uint64
    lib.lg_post_physics_transition.argtypes = [vp, vp, vp, f32, vp, vp, vp]
    lib.lg_post_physics_transition.restype = C.c_int
    lib.lg_extra_obs_info.argtypes = [vp, C.POINTER(i32), C.POINTER(vp)]
    lib.lg_extra_obs_info.restype = C.c_int
    lib.lg_sensor_rig_create.argtypes = [vp, vp, C.POINTER(lg_sensor_raycaster), C.POINTER(lg_sensor_camera)]
    lib.lg_sensor_rig_create.restype = vp
    lib.lg_sensor_rig_destroy.argtypes = [vp]
    lib.lg_sensor_rig_destroy.restype = None
    lib.lg_sensor_rig_counter.argtypes = [vp]
    lib.lg_sensor_rig_counter.restype = i64
    lib.lg_sensor_rig_set_counter.argtypes = [vp, i64]
    lib.lg_sensor_rig_set_counter.restype = C.c_int
    lib.lg_sensor_step_transition.argtypes = [vp, vp, vp, vp, f32, vp, vp, vp]
    lib.lg_sensor_step_transition.restype = C.c_int
    lib.lg_runner_collect_sensors.argtypes = [vp, vp, vp, vp, vp, vp, u64, u64, i32, f32, f32, i32, C.POINTER(lg_rollout), C.POINTER(lg_rollout_hidden),
                                              vp, vp, vp, vp, C.POINTER(lg_runner_hooks), vp]
    lib.lg_runner_collect_sensors.restype = C.c_int
    lib.lg_estimation_rows.argtypes = [vp, i32, i64, vp, vp, vp, vp, i64, i32, vp, vp, vp, vp]
    lib.lg_estimation_rows.restype = C.c_int
    lib.lg_collect_estimation.argtypes = [vp, vp, vp, i32, C.POINTER(lg_estimation_out), C.POINTER(lg_estimation_nets), vp]
    lib.lg_collect_estimation.restype = C.c_int
    return lib


class lg_estimation_driver(C.Structure):
    """include/lgrunner_estimator.h: who moves the robot during an estimation collection; the four last members exist to be refused by name."""
    _fields_ = [("actions", C.c_void_p), ("actor", C.c_void_p), ("memory", C.c_void_p), ("h", C.c_void_p), ("c", C.c_void_p), ("normalizer", C.c_void_p),
                ("normalizer_training", i32), ("critic", C.c_void_p), ("std", C.c_void_p), ("privileged_observations", C.c_void_p)]


class lg_estimation_stats(C.Structure):
    """include/lgrunner_estimator.h: the per-step means, the four per-ray rows and the kernel's workspace."""
    _fields_ = [(k, C.c_void_p) for k in ("mse", "mae", "ray_sq_error", "ray_abs_error", "ray_bias", "ray_max_error", "workspace")] + \
        [("workspace_floats", C.c_int64)]


def declare_runner_estimator(lib):
    """Prototypes of the terrain-estimator runner's device side (include/lgrunner_estimator.h), same library."""
    vp, i64 = C.c_void_p, C.c_int64
    lib.lg_estimation_errors_workspace.argtypes = [i64, i32]
    lib.lg_estimation_errors_workspace.restype = i64
    lib.lg_estimation_errors.argtypes = [vp, vp, i32, i64, i32, C.POINTER(lg_estimation_stats), vp]
    lib.lg_estimation_errors.restype = C.c_int
    lib.lg_runner_collect_estimation.argtypes = [vp, C.POINTER(lg_estimation_driver), i32, C.POINTER(lg_estimation_out), C.POINTER(lg_estimation_nets),
                                                 C.POINTER(lg_estimation_stats), vp]
    lib.lg_runner_collect_estimation.restype = C.c_int
    return lib


# ---------------------------------------------------------------------------------------------------------------------------------- the units
Unit =collections.namedtuple("Unit", "declare headers")

# One row per `declare_*` function: the headers under include/ whose prototypes it mirrors.  Everything else about a unit is derived: its symbols
# are what the function sets (`symbols`), its structs are the `typedef struct lg_...` names of its headers, found here by name.  A new header
# costs its `declare_x`, a row here and the refusal table of its test file; tests/test_abi_units.py holds every row to the same checks.
UNITS = {
    "product": Unit(declare_product, ("lgstep.h",)),
    "policy": Unit(declare_policy, ("lgpolicy.h",)),
    "policy_wide": Unit(declare_policy_wide, ("lgpolicy_wide.h", "lgpolicy_wide_memory.h")),
    "train": Unit(declare_train, ("lgtrain.h",)),
    "train_symmetry": Unit(declare_train_symmetry, ("lgtrain_symmetry.h",)),
    "train_recurrent": Unit(declare_train_recurrent, ("lgtrain_recurrent.h",)),
    "distill_train": Unit(declare_distill_train, ("lgdistill.h",)),
    "distill_rtrain": Unit(declare_distill_rtrain, ("lgdistill_recurrent.h",)),
    "estimator_train": Unit(declare_estimator_train, ("lgestimator_train.h",)),
    "estimator_train_bf16": Unit(declare_estimator_train_bf16, ("lgestimator_train_bf16.h",)),
    "runner": Unit(declare_runner, ("lgrunner.h",)),
    "runner_privileged": Unit(declare_runner_privileged, ("lgrunner_privileged.h",)),
    "runner_distill": Unit(declare_runner_distill, ("lgrunner_distill.h",)),
    "sensors": Unit(declare_sensors, ("lgsensors.h",)),
    "runner_estimator": Unit(declare_runner_estimator, ("lgrunner_estimator.h",)),
}


class _Recorder:
    """Stands in for the library: keeps every function a `declare_*` touches, with the prototype it is given."""

    def __init__(self):
        self.functions = {}

    def __getattr__(self, name):
        return self.functions.setdefault(name, types.SimpleNamespace(argtypes=None, restype=C.c_int))


@functools.lru_cache(maxsize=None)
def _recorded(declare):
    rec = _Recorder()
    declare(rec)
    return rec.functions


def prototypes(unit):
    """name -> (argtypes, restype) record of every function the unit's `declare_*` sets, in the order it sets them.  No library needed.  (Kept per
    declare function, not per unit name: whoever replaces a row of `UNITS` gets that row's own record.)"""
    return _recorded(UNITS[unit].declare)


def symbols(unit):
    """The entry points of a unit: what its `declare_*` declares."""
    return list(prototypes(unit))


def declare(lib, *units):
    """Sets the prototypes of the named units on `lib`, each at most once per library object; every unit: `declare(lib, *UNITS)`."""
    done = lib.__dict__.setdefault("_lg_units", set())
    for unit in units:
        if unit not in done:
            UNITS[unit].declare(lib)
            done.add(unit)
    return lib


PRODUCT_SYMBOLS, POLICY_SYMBOLS, TRAIN_SYMBOLS = symbols("product"), symbols("policy"), symbols("train")
