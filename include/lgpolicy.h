/* lgpolicy.h — C ABI of the rollout-collection side of the training loop: the
 * actor / critic MLP forward passes and action sampling of rsl_rl's PPO.act, and RolloutStorage.compute_returns.
 * Library: extended_legged_gym_amd/csrc/liblgstep.so (same library as lgstep.h).  Device pointers unless marked HOST;
 * every call is asynchronous on the caller's hipStream_t; 0 / negative status as in lgstep.h.
 *
 * Reference (vendored rsl_rl): modules/actor_critic.py:38-66 (nn.Sequential of Linear + activation), :120-136
 * (update_distribution / act / get_actions_log_prob / act_inference / evaluate), algorithms/ppo.py:147-159 (PPO.act),
 * storage/rollout_storage.py:145-167 (compute_returns). */
#ifndef LGPOLICY_H
#define LGPOLICY_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define LG_MLP_MAX_LAYERS 8
enum lg_activation { LG_ACT_ELU = 0, LG_ACT_RELU = 1, LG_ACT_TANH = 2, LG_ACT_LRELU = 3 /* slope 0.01 */, LG_ACT_SELU = 4 };

typedef struct lg_mlp lg_mlp;

/* One nn.Sequential(Linear, act, ..., Linear) (actor_critic.py:42-66).  dims[0 .. num_layers]: input width, hidden widths,
 * output width; weights[l] is Linear.weight of layer l, (dims[l+1], dims[l]) row-major, biases[l] (dims[l+1]) — HOST
 * pointers, re-tiled for the matrix cores and uploaded.  Every width, the input's included, is 1..512; an input row of up to 2048
 * columns: lg_mlp_create_wide of lgpolicy_wide.h, whose handles every entry point below that runs the MLP on the caller's row takes as they are. */
lg_mlp* lg_mlp_create(int32_t num_layers, const int32_t* dims, const float* const* weights, const float* const* biases,
                      int32_t activation, int device_id);
void lg_mlp_destroy(lg_mlp* mlp);
/* The error channel of EVERY entry point of this header: the calling thread's last message, the same whether `mlp` is a handle or NULL.
 * Each non-zero status (and each NULL from a create function) leaves a message "<entry point the caller called>: <reason>" -- a failure
 * inside a collector names the collector, not the act it ran.  The pointer stays valid until the thread's next failing call. */
const char* lg_mlp_last_error(lg_mlp* mlp);

/* y (n, dims[L]) = mlp(x (n, dims[0])): all layers in one launch, activations stay in LDS, fp32 MFMA
 * (actor(observations) / critic(observations), actor_critic.py:129-136). */
int lg_mlp_forward(lg_mlp* mlp, const float* x, int64_t n, float* y, void* stream);

/* PPO.act (ppo.py:147-159) for a feed-forward ActorCritic: one launch evaluates both networks;
 *   action_mean = actor(obs); actions = action_mean + std * z, z ~ N(0,1) from Philox4x32-10 keyed by (seed, call, row);
 *   actions_log_prob = sum_a [-(a - mean)^2 / (2 std^2) - log std - log sqrt(2 pi)]; values = critic(critic_obs).
 * std: (num_actions) device vector (the `std` parameter, or exp(log_std)).  Outputs: actions, action_mean (n, A),
 * actions_log_prob (n), values (n, critic out width).  deterministic != 0: actions = action_mean (act_inference). */
int lg_policy_act(lg_mlp* actor, lg_mlp* critic, const float* obs, const float* critic_obs, int64_t n, const float* std,
                  uint64_t seed, uint64_t call, int32_t deterministic, float* actions, float* action_mean,
                  float* actions_log_prob, float* values, void* stream);

/* RolloutStorage.compute_returns (rollout_storage.py:145-167): GAE over T transitions of n envs, all (T, n) row-major f32
 * (dones: 0 / 1 as f32), last_values (n); writes returns and advantages (T, n); normalize != 0: advantages =
 * (adv - mean) / (std + 1e-8) with the unbiased std over all T*n entries (torch.std).  T*n = 1: the std of one entry is
 * taken as 0 and the one advantage comes back as 0 (torch.std, and so the reference, gives NaN there); returns are not touched. */
int lg_compute_returns(const float* rewards, const float* dones, const float* values, const float* last_values, int32_t T,
                       int64_t n, float gamma, float lam, int32_t normalize, float* returns, float* advantages, void* stream);

/* The collection loop of OnPolicyRunner.learn (runners/on_policy_runner.py:395-445) for a feed-forward policy, without
 * returning to the host between steps: for t in [0, T):
 *     observations[t] = env obs;  PPO.act (ppo.py:147-159) -> actions[t], values[t], actions_log_prob[t], mu[t], sigma[t];
 *     one lg_step of the env with actions[t];   PPO.process_env_step (ppo.py:161-183): rewards[t] = rew + gamma * values[t] * time_outs,
 *     dones[t] = reset_buf
 * then last_values = critic(env obs) (ppo.py:186-190) and, when returns / advantages are given, compute_returns.
 * Rows are laid out as RolloutStorage holds them (rollout_storage.py:47-76), (T, n, .) row-major f32 (dones as 0 / 1).
 * Sampling call t uses Philox call number first_call + t, so the loop draws exactly what T separate lg_policy_act calls
 * with calls first_call .. first_call + T - 1 draw.  The policy sees the env's obs_buf as both actor and critic input
 * (no privileged observations).  Everything is enqueued on `stream`; nothing is synchronised. */
struct lg_ctx;
typedef struct lg_rollout {
  float* observations;       /* (T, n, num_obs) */
  float* actions;            /* (T, n, A) */
  float* rewards;            /* (T, n) */
  float* dones;              /* (T, n) */
  float* values;             /* (T, n) */
  float* actions_log_prob;   /* (T, n) */
  float* mu;                 /* (T, n, A) */
  float* sigma;              /* (T, n, A) */
  float* last_values;        /* (n) */
  float* returns;            /* (T, n) or NULL */
  float* advantages;         /* (T, n) or NULL */
} lg_rollout;
int lg_collect_rollout(struct lg_ctx* env, lg_mlp* actor, lg_mlp* critic, const float* std, uint64_t seed, uint64_t first_call,
                       int32_t T, float gamma, float lam, int32_t normalize_advantage, const lg_rollout* out, void* stream);

/* ---- recurrent actor-critic: the nn.LSTM / nn.GRU "memory" in front of each MLP (vendored rsl_rl: networks/memory.py:16-51,
 * modules/actor_critic_recurrent.py:16-85; selected by runner.policy_class_name = "ActorCriticRecurrent" with the knobs rnn_type,
 * rnn_hidden_size, rnn_num_layers of legged_robot_config.py:279).  Inference / collection here; the batch mode of PPO.update (the reference's
 * act(obs, masks=, hidden_states=) over padded trajectories) is the recurrent trainer of lgtrain_recurrent.h, which walks the same rows unpadded.
 *
 * One memory step for n rows, ONE launch per memory layer (the actor's and the critic's memory share a launch when they step together):
 *     gates = W_ih x + b_ih + W_hh h + b_hh                                     (n, G H), one fp32 MFMA k-chain over [x ; h]
 *     LSTM (torch's gate order i, f, g, o):  c' = sig(f) c + sig(i) tanh(g);   h' = sig(o) tanh(c')
 *     GRU  (r, z, n):  n = tanh(W_in x + b_in + r * (W_hn h + b_hn));          h' = (1 - z) n + z h
 * State: h (and c for an LSTM; NULL for a GRU), (num_layers, n, hidden) row-major f32 on the device, owned by the caller and updated IN
 * PLACE (a workgroup owns whole rows and reads them before it writes them).  Layer l > 0 reads the h' of layer l - 1. */
enum lg_rnn_type { LG_RNN_LSTM = 0, LG_RNN_GRU = 1 };
typedef struct lg_rnn lg_rnn;

/* One Memory.rnn (memory.py:20-22).  w_ih[l]: weight_ih_l{l} (G hidden, input or hidden), w_hh[l]: weight_hh_l{l} (G hidden, hidden),
 * b_ih[l] / b_hh[l]: (G hidden) -- HOST pointers in torch's layout, re-tiled for the matrix cores and uploaded.  Limits: input 1..512,
 * hidden 1..512 (any value), 1..4 layers; NULL + a message in lg_mlp_last_error(NULL) otherwise. */
lg_rnn* lg_rnn_create(int32_t type, int32_t num_layers, int32_t input, int32_t hidden, const float* const* w_ih, const float* const* w_hh,
                      const float* const* b_ih, const float* const* b_hh, int device_id);
void lg_rnn_destroy(lg_rnn* rnn);

/* The host re-tiling of one layer, a pure function (no device): tiled[((c (nb + 1) + b) G + g) 64 + lane][s] = Wcat[g hidden + 16 c + (lane & 15)][16 b + 4 s + (lane >> 4)]
 * with Wcat[:, 0 .. input) = w_ih, Wcat[:, Ip .. Ip + hidden) = w_hh, zero elsewhere; Ip = input rounded up to 16, nb = (Ip + hidden rounded up to 16) / 16 blocks
 * (block nb of every chunk is all zero), chunks c of 16 hidden units.  Returns the number of floats of `tiled` (HOST; NULL: only the count), negative on bad arguments. */
int64_t lg_rnn_tile_weights(int32_t type, int32_t input, int32_t hidden, const float* w_ih, const float* w_hh, float* tiled);

/* Memory.forward in inference mode (memory.py:31-33: out, hidden_states = rnn(input.unsqueeze(0), hidden_states)) for all layers.
 * x (n, input); reset (n) f32 0 / 1 or NULL: rows with reset != 0 enter the step with h = c = 0 (Memory.reset(dones), memory.py:45-51,
 * folded into the next step); out (n, hidden) or NULL: a copy of the top layer's h'. */
int lg_rnn_step(lg_rnn* rnn, const float* x, int64_t n, float* h, float* c, const float* reset, float* out, void* stream);

/* Memory.reset(dones) on its own (memory.py:45-51; PPO.process_env_step resets AFTER the step, ppo.py:188): rows with dones != 0 of every layer's h / c = 0. */
int lg_rnn_reset_rows(lg_rnn* rnn, float* h, float* c, const float* dones, int64_t n, void* stream);

/* PPO.act (ppo.py:147-159) for an ActorCriticRecurrent (actor_critic_recurrent.py:66-80): both memories step (one launch per layer), then
 * lg_policy_act on the top layers' h'.  Sampling is lg_policy_act's: for equal (seed, call, row) a recurrent and a feed-forward policy
 * draw the same standard normals.  h_a / c_a, h_c / c_c: the actor / critic memory state, in place; reset as in lg_rnn_step (both memories). */
int lg_policy_act_recurrent(lg_rnn* mem_a, lg_mlp* actor, lg_rnn* mem_c, lg_mlp* critic, const float* obs, const float* critic_obs, int64_t n,
                            const float* std, uint64_t seed, uint64_t call, int32_t deterministic, float* h_a, float* c_a, float* h_c, float* c_c,
                            const float* reset, float* actions, float* action_mean, float* actions_log_prob, float* values, void* stream);

/* The rows RolloutStorage._save_hidden_states keeps (rollout_storage.py:123-140): per memory and state tensor (T, num_layers, n, hidden),
 * the state BEFORE step t's act (ppo.py:148-149).  c_a / c_c NULL for a GRU. */
typedef struct lg_rollout_hidden {
  float* h_a;
  float* c_a;
  float* h_c;
  float* c_c;
} lg_rollout_hidden;

/* lg_collect_rollout for a recurrent policy (on_policy_runner.py:395-445 with ppo.py:147-192): per step t the hidden rows are saved, both
 * memories and MLPs run, the env steps, and both memories are reset on dones[t] (ppo.py:188).  last_values = policy.evaluate(last obs)
 * (ppo.py:190-192) goes through Memory.forward as in the reference, so it ADVANCES the critic memory once more: the next iteration's
 * first evaluate sees the same observation a second time.  h_a .. c_c: the live memory state, left as the loop leaves it. */
int lg_collect_rollout_recurrent(struct lg_ctx* env, lg_rnn* mem_a, lg_mlp* actor, lg_rnn* mem_c, lg_mlp* critic, const float* std, uint64_t seed,
                                 uint64_t first_call, int32_t T, float gamma, float lam, int32_t normalize_advantage, const lg_rollout* rows,
                                 const lg_rollout_hidden* hidden, float* h_a, float* c_a, float* h_c, float* c_c, void* stream);

/* ---- teacher-student distillation (vendored rsl_rl: algorithms/distillation.py:89-105, modules/student_teacher.py:93-109,
 * modules/student_teacher_recurrent.py:71-95; selected by runner.policy_class_name = "StudentTeacher" / "StudentTeacherRecurrent" with
 * algorithm_class_name = "Distillation").  Collection only: Distillation.update (distillation.py:107-153) stays in PyTorch.
 *
 * lg_obs_history_step: the observation-history layer of a student env, AnymalStudent.compute_observations (envs/anymal_c/anymal.py:336-383)
 * after reset_idx zeroed the rows of the envs that were reset (:330-334), in ONE launch, on an (n, H, W) history IN PLACE:
 *     1. rows with dones != 0 are zeroed;   2. slots shift by one, oldest out;   3. slot 0 = obs[row, 0 .. W) (obs has row stride obs_stride >= W);
 *     4. history[row, k] += (2 u - 1) * noise_scale[k] for ALL k = slot * W + column in [0, H W): the reference adds the noise to a view of the history,
 *        so older slots collect a fresh draw every step;   5. obs_out[row, k] = clamp(history[row, k], -clip, clip); the stored history stays unclipped.
 * u: inject_u (n, H W) when given (the checker mode: the result then equals the torch function bit for bit -- 2 u, - 1, * scale, + are four rounded fp32
 * operations, no FMA); otherwise Philox4x32-10 with counter (row_lo, row_hi, 0x80000000 | k, call_lo ^ (call_hi * 0x9E3779B9)) and key (seed_lo, seed_hi),
 * u = u01 of its first word (the generator of lg_policy_act; bit 31 of the third counter word keeps the draws apart from lg_policy_act's for equal
 * seed and call).  noise_scale NULL: no noise.  dones (n) f32 0 / 1 or NULL; obs_out (n, H W) or NULL; clip > 0 (INFINITY: no clip).
 * LG_ERR_INVALID for H < 1, W < 1, obs_stride < W, clip <= 0 or a NULL history / obs (message in lg_mlp_last_error(NULL)). */
int lg_obs_history_step(float* history, int64_t n, int32_t H, int32_t W, const float* obs, int64_t obs_stride, const float* dones,
                        const float* noise_scale, const float* inject_u, uint64_t seed, uint64_t call, float clip, float* obs_out, void* stream);

/* Distillation.act (distillation.py:89-96) for a StudentTeacher (student_teacher.py:93-109): one launch of lg_policy_act's kernel with the teacher
 * in the second slot and no log-prob:
 *   action_mean = student(obs); actions = action_mean + std * z (deterministic != 0: actions = action_mean); teacher_actions = teacher(teacher_obs).
 * For equal (seed, call, row) z is what lg_policy_act draws.  Both networks must end in the same width A <= 32; action_mean (n, A) or NULL. */
int lg_distill_act(lg_mlp* student, lg_mlp* teacher, const float* obs, const float* teacher_obs, int64_t n, const float* std, uint64_t seed,
                   uint64_t call, int32_t deterministic, float* actions, float* action_mean, float* teacher_actions, void* stream);

/* The same for a StudentTeacherRecurrent (student_teacher_recurrent.py:78-89): the student's memory steps, and the teacher's when it has one (both
 * in one launch per layer when their depths agree, as in lg_policy_act_recurrent); mem_t NULL: the teacher MLP reads teacher_obs directly
 * (teacher_recurrent = False; h_t / c_t are then ignored).  h_s / c_s, h_t / c_t: memory state, in place; reset as in lg_rnn_step. */
int lg_distill_act_recurrent(lg_rnn* mem_s, lg_mlp* student, lg_rnn* mem_t, lg_mlp* teacher, const float* obs, const float* teacher_obs, int64_t n,
                             const float* std, uint64_t seed, uint64_t call, int32_t deterministic, float* h_s, float* c_s, float* h_t, float* c_t,
                             const float* reset, float* actions, float* action_mean, float* teacher_actions, void* stream);

/* The rows RolloutStorage keeps in "distillation" mode (rollout_storage.py:65-67, 102-104, 170-182), (T, n, .) row-major f32. */
typedef struct lg_distill_rollout {
  float* observations;              /* (T, n, O_s)  the student's */
  float* privileged_observations;   /* (T, n, O_t)  the teacher's: the env's observation row */
  float* actions;                   /* (T, n, A)    the student's sampled actions */
  float* privileged_actions;        /* (T, n, A)    the teacher's */
  float* rewards;                   /* (T, n)       the env's raw reward: no time-out bootstrap (distillation.py:98-101) */
  float* dones;                     /* (T, n) */
  float* last_observations;         /* (n, O_s) or NULL: the student's observation after the last step */
} lg_distill_rollout;

/* The history layer between the env's row and the student (lg_obs_history_step): step t of a collection uses noise call first_call + t and,
 * when given, the uniforms inject_u[t]. */
typedef struct lg_obs_history {
  float* history;             /* (n, H, W), in place */
  int32_t H, W;
  const float* noise_scale;   /* (H W) or NULL: no noise */
  float clip;
  uint64_t noise_seed;
  const float* inject_u;      /* (T, n, H W) or NULL: Philox */
} lg_obs_history;

/* The collection loop of OnPolicyRunner.learn (on_policy_runner.py:395-445) with Distillation.act / process_env_step (distillation.py:89-105), without
 * returning to the host between steps: for t in [0, T):
 *     lg_distill_act on observations[t], privileged_observations[t] -> actions[t], privileged_actions[t]   (Philox call first_call + t);
 *     one env step (lg_step_transition without a value row: rewards[t] = the env's reward, dones[t] = reset_buf), the next teacher row written
 *     straight into privileged_observations[t + 1];
 *     the student's next row: lg_obs_history_step on `history` -> observations[t + 1] (last_observations after the last step).
 * Row 0: privileged_observations[0] = the env's observation row, observations[0] = clamp(history, +-clip).  history NULL: the student sees the first
 * O_s columns of the teacher's row.  O_s = the student's input width, O_t = the env's observation width = the teacher's input width. */
int lg_collect_distillation(struct lg_ctx* env, lg_mlp* student, lg_mlp* teacher, const float* std, uint64_t seed, uint64_t first_call, int32_t T,
                            const lg_obs_history* history, const lg_distill_rollout* rows, void* stream);

/* The same for a StudentTeacherRecurrent; both memories are reset on dones[t] after each step (distillation.py:105).  h_s .. c_t: the live memory
 * state, left as the loop leaves it.  h_s0 .. c_t0 (each (L, n, hidden), or NULL): the state BEFORE step 0 -- distillation mode keeps no per-step
 * hidden rows (Distillation.act never sets transition.hidden_states); this is what seeds policy.reset(hidden_states=...) for the update. */
int lg_collect_distillation_recurrent(struct lg_ctx* env, lg_rnn* mem_s, lg_mlp* student, lg_rnn* mem_t, lg_mlp* teacher, const float* std,
                                      uint64_t seed, uint64_t first_call, int32_t T, const lg_obs_history* history, const lg_distill_rollout* rows,
                                      float* h_s0, float* c_s0, float* h_t0, float* c_t0, float* h_s, float* c_s, float* h_t, float* c_t, void* stream);

/* ---- terrain estimator: depth image + base velocities -> the ray caster's distances (vendored rsl_rl: modules/terrain_estimator.py:13-218;
 * trained by algorithms/distillation.py:190-433 through runners/terrain_estimator_runner.py).  Inference / collection here; the update
 * (EstimatorDistillation.update, distillation.py:277-332) is lgestimator_train.h, which trains the images of these handles in place.
 *
 * lg_conv_encoder: TerrainEstimator._build_cnn_encoder (terrain_estimator.py:80-109), forward only, fp32, for a (height, width) image:
 *     Conv2d(1, 32, k5, s2, p2) act  Conv2d(32, 64, k3, s2, p1) act  Conv2d(64, 128, k3, s2, p1) act  Conv2d(128, 64, k3, s1, p1) act
 *     AdaptiveAvgPool2d((4, 4)) Flatten  Linear(1024, 128) act  Linear(128, out_dim) act
 * act: the module's one shared activation (:44-51): LG_ACT_ELU, LG_ACT_RELU or LG_ACT_TANH.  weights[6] / biases[6]: HOST pointers in torch's
 * layouts, in the order of the layers above (Sequential indices 0 2 4 6 10 12): conv (C_out, C_in, kh, kw), linear (out, in).  Every layer is an
 * implicit GEMM on the fp32 matrix cores over rows = (env, output pixel); no atomics, no split reductions: equal inputs give equal bits.
 * Limits: 8 <= height, width <= 128, 1 <= out_dim <= 512; NULL + a message in lg_mlp_last_error(NULL) beyond them.  The encoder owns its
 * workspaces (the intermediate maps of all n rows); they grow on the first call with a larger n, which waits for the device once.  Calls on
 * one encoder must not overlap on different streams. */
typedef struct lg_conv_encoder lg_conv_encoder;
lg_conv_encoder* lg_conv_encoder_create(int32_t height, int32_t width, int32_t out_dim, int32_t activation, const float* const* weights,
                                        const float* const* biases, int device_id);
void lg_conv_encoder_destroy(lg_conv_encoder* enc);

/* The encoder's precision mode.  LG_PREC_F32 is lg_conv_encoder_create.  LG_PREC_BF16 (opt-in, inference on the bf16 matrix cores,
 * v_mfma_f32_16x16x32_bf16): all six layers take bf16 operands and accumulate in fp32.  Rounding points, each fp32 -> bf16 to nearest even:
 * the weights once at create time (lg_conv_tile_weights_bf16), the depth image on its way into conv 1 (zero padding stays exact), and the
 * output of stages 1-6 (conv 1-4, pool + flatten, linear 1) as it is stored -- the workspaces hold bf16.  Biases stay fp32 and are added to the
 * fp32 accumulator, the activation is evaluated in fp32, the pooling averages in fp32, and linear 2 writes fp32 features where the fp32 path
 * writes them.  One fixed-order accumulation per output, no atomics, no split K: equal inputs give equal bits.  Same limits, same refusals;
 * an unknown precision returns NULL with a message in lg_mlp_last_error(NULL), before any device is touched.  forward, forward_stages,
 * stage_shape and lg_estimator_step take an encoder of either mode; the combination layer, memory and decoder stay fp32.
 * lg_conv_encoder_precision: the mode of an encoder, LG_ERR_INVALID for NULL. */
#define LG_PREC_F32 0
#define LG_PREC_BF16 1
lg_conv_encoder* lg_conv_encoder_create_precision(int32_t height, int32_t width, int32_t out_dim, int32_t activation, const float* const* weights,
                                                  const float* const* biases, int device_id, int32_t precision);
int32_t lg_conv_encoder_precision(const lg_conv_encoder* enc);

/* The host re-tiling of one layer, a pure function (no device).  With K = kh kw c_in and tap index k = (ky kw + kx) c_in + ci (channel fastest:
 * the kernels keep activations (env, y, x, channel)), nkb = (K rounded up to 64) / 16 blocks and nch = (c_out rounded up to 64) / 16 chunks:
 *     tiled[((c nkb + b) 64 + lane) 4 + s] = weight[16 c + (lane & 15)][ci][ky][kx]   for k = 16 b + 4 s + (lane >> 4),   zero for k >= K or a channel >= c_out.
 * A linear layer (out, in) is c_out = out, c_in = in, kh = kw = 1.  Returns the number of floats of `tiled` (HOST; NULL: only the count);
 * LG_ERR_INVALID for c_out outside 1..512, c_in outside 1..1024, kh / kw outside 1..15, or a NULL weight with a non-NULL `tiled`. */
int64_t lg_conv_tile_weights(int32_t c_out, int32_t c_in, int32_t kh, int32_t kw, const float* weight, float* tiled);

/* The same for LG_PREC_BF16, in the operand order of v_mfma_f32_16x16x32_bf16.  With K and k as above, nks = (K rounded up to 32) / 32 k-steps and
 * nch = (c_out rounded up to 64) / 16 chunks:
 *     tiled[((c nks + s) 64 + lane) 8 + j] = bf16(weight[16 c + (lane & 15)][ci][ky][kx])   for k = 32 s + 8 (lane >> 4) + j,   zero for k >= K or a channel >= c_out,
 * bf16(): the upper 16 bits of the fp32 value rounded to nearest even.  Returns the number of 16-bit elements of `tiled` (HOST; NULL: only the
 * count); LG_ERR_INVALID as lg_conv_tile_weights. */
int64_t lg_conv_tile_weights_bf16(int32_t c_out, int32_t c_in, int32_t kh, int32_t kw, const float* weight, uint16_t* tiled);

/* features (n, out_dim) = depth_encoder(depth.unsqueeze(1)) (terrain_estimator.py:164-167).  Image e starts at depth + e * depth_stride and is
 * (height, width) row-major: depth_stride = buffer_len * height * width reads the latest frame of the camera's (n, buffer_len, height, width)
 * FIFO in place (depth_buffer[:, -1]).  LG_ERR_INVALID for n <= 0, a NULL pointer or depth_stride < height * width; nothing is launched then. */
int lg_conv_encoder_forward(lg_conv_encoder* enc, const float* depth, int64_t depth_stride, int64_t n, float* features, void* stream);

/* The encoder cut after its first `stages` stages, for checking a layer on its own.  Stages 1..7: conv 1-4 (each with its activation), pool + flatten,
 * linear 1, linear 2.  It runs the launches lg_conv_encoder_forward runs for those stages -- same kernels, grids, workspaces and order, through the same
 * code -- and copies the last one's rows to `out` (device, n x count floats, asynchronous on `stream`) in the layout the kernels keep:
 *     conv stage: (n, H_out, W_out, C_out), channel last;   pool: (n, 1024), channel major (torch's Flatten);   linear 1: (n, 128);   linear 2: (n, out_dim).
 * On an LG_PREC_BF16 encoder the bf16 rows of stages 1-6 are expanded exactly to fp32 on the way to `out`, in the same layouts.
 * stages = 7 writes what lg_conv_encoder_forward writes, bit for bit.  LG_ERR_INVALID as there, and for stages outside 1..7; nothing is launched then.
 * lg_conv_encoder_stage_shape: the floats of one row of stage `stage`'s output (the `count` above), and through h / w / c (each may be NULL) the map
 * (H_out, W_out, C_out) of a conv stage, (1, 1, width) of the others; LG_ERR_INVALID for a NULL encoder or a stage outside 1..7.  No device work. */
int64_t lg_conv_encoder_stage_shape(const lg_conv_encoder* enc, int32_t stage, int32_t* h, int32_t* w, int32_t* c);
int lg_conv_encoder_forward_stages(lg_conv_encoder* enc, const float* depth, int64_t depth_stride, int64_t n, int32_t stages, float* out, void* stream);

/* enabled != 0: the activation also follows the LAST layer of the network, as nn.Sequential(Linear, act) has it -- the estimator's combination_mlp
 * (terrain_estimator.py:58-61).  Networks keep a linear last layer unless this is called. */
int lg_mlp_set_output_activation(lg_mlp* mlp, int32_t enabled);

/* TerrainEstimator.forward in single-step mode (terrain_estimator.py:162-198):
 *     features = encoder(depth);  x = combine(cat[features, proprio]);  memory step on x (lg_rnn_step: h / c in place, rows with reset != 0 enter
 *     with zero state);  predictions (n, decoder out) = decoder(h' of the top layer).
 * combine: an lg_mlp of ONE layer, (out_dim + P) -> the memory's input width, with lg_mlp_set_output_activation enabled; P = the width of a
 * proprio row (n, P) (base_lin_vel, base_ang_vel: 6).  decoder: an lg_mlp whose input is the memory's hidden width.  LG_ERR_INVALID with a
 * message in lg_mlp_last_error(NULL) when the widths do not chain, n <= 0, or a pointer is NULL (c may be NULL for a GRU, reset always). */
int lg_estimator_step(lg_conv_encoder* enc, lg_mlp* combine, lg_rnn* mem, lg_mlp* decoder, const float* depth, int64_t depth_stride,
                      const float* proprio, int64_t n, float* h, float* c, const float* reset, float* predictions, void* stream);

/* ---- the sampling planner's arithmetic around rollout_batch.
 * The reference's planner envs (envs/batch_rollout/robot_traj_grad_sampling.py:210-280) hand `rollout_batch` as a callback to the
 * optimiser of the external package `traj_sampling` (imported at :18, not in the reference tree, no pinned version): per diffusion step
 * it perturbs the node trajectories, interpolates nodes -> dense plans, rolls the plans out, and re-weights the samples.  Restated here
 * from the published algorithm that package implements (DIAL-MPC: Xue et al., "Full-Order Sampling-Based MPC for Torque-Level
 * Locomotion Control via Diffusion-Style Annealing", 2024, with the MPPI update of its reference code; config names:
 * robot_traj_grad_sampling_config.py:44-71 -- num_samples, temp_sample, horizon_samples, horizon_nodes, update_method "mppi"):
 *
 * lg_plan_from_nodes: plans[i, h, a] = sum_k phi[h, k] * nodes[i, k, a]     (n, K, A) -> (n, H, A); phi (H, K) holds the interpolation
 *     weights of the node -> sample-time spline (a linear operator: the host builds it once, linear or cubic);
 * lg_mppi_update: for main env m with sample rows i in [m R, (m + 1) R):
 *     r_i = mean_h rewards[i, h];   z_i = (r_i - mean_i r) / std_i r   (population std; all-equal rewards: z = 0);
 *     weights[i] = softmax_i(z_i / temperature);   new_nodes[m, k, a] = sum_i weights[i] nodes[i, k, a].
 * All pointers are device pointers, row-major f32; asynchronous on `stream`. */
int lg_plan_from_nodes(const float* nodes, const float* phi, int64_t n, int32_t K, int32_t H, int32_t A, float* plans, void* stream);
int lg_mppi_update(const float* rewards, const float* nodes, int32_t num_main, int32_t R, int32_t H, int32_t K, int32_t A,
                   float temperature, float* new_nodes, float* weights, void* stream);


/* The diffusion passes of one control step WITHOUT a return to the host between them (round 6; SURVEY s8(f) rank 4 "sampler glue fused":
 * `optimize_all_trajectories`, robot_traj_grad_sampling.py:226-247, which in the reference is a Python loop of sample -> node2u -> rollout_batch -> softmax per pass).
 *
 * lg_mppi_sample_plans: the samples of one pass.  Row i = m R + s of the launch (main env m, sample s):
 *     nodes[i, k, a] = mean[m, k, a] + sigma_scale * sigma_nodes[k] * z(i, k A + a),   z = 0 for s = 0 (sample 0 is the mean itself), else N(0, 1):
 *         Philox4x32-10 with counter (i, call_lo, (k A + a) >> 1, call_hi) and key (seed_lo, seed_hi), Box-Muller on its first two words
 *         (u1 = max(u01(o0), 2^-24), u2 = u01(o1); cosine for even k A + a, sine for odd) -- the generator of lg_policy_act;
 *     plans[i, h, a] = sum_k phi[h, k] * nodes[i, k, a]                        (what lg_plan_from_nodes computes from the same nodes).
 * lg_planner_diffuse: n_diffuse passes of { lg_mppi_sample_plans (sigma_scale = traj_diffuse_factor^pass, call = call0 + pass) -> lg_rollout_batch on `ctx`
 *     (sync main -> rollout, H rollout steps, sync) -> lg_mppi_update -> mean }, enqueued by ONE call; `mean` (M, K, A) is updated in place, `weights` (M, R) and
 *     `rewards` (M R, H) hold the last pass's.  nodes / plans / rewards are caller-provided workspaces of (M R, K, A), (M R, H, A), (M R, H) floats.
 *     env_ids: the n = M R rollout envs of `ctx` in row order (RobotBatchRollout.rollout_env_indices); A must be the robot's DOF count. */
struct lg_ctx;
int lg_mppi_sample_plans(const float* mean, const float* sigma_nodes, float sigma_scale, const float* phi, int32_t num_main, int32_t R, int32_t K, int32_t H,
                         int32_t A, uint64_t seed, uint64_t call, float* nodes, float* plans, void* stream);
int lg_planner_diffuse(struct lg_ctx* ctx, float* mean, const float* sigma_nodes, const float* phi, int32_t num_main, int32_t R, int32_t K, int32_t H, int32_t A,
                       int32_t n_diffuse, float traj_diffuse_factor, float temperature, uint64_t seed, uint64_t call0, const int32_t* env_ids,
                       int32_t rollouts_per_main, float pos_drift, float* nodes, float* plans, float* rewards, float* weights, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LGPOLICY_H */
