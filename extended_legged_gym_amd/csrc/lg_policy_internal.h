// lg_policy_internal.h — the host plumbing lg_policy.hip, lg_planner.hip and lg_estimator.hip share beyond the C ABI: the one error channel
// (the thread's message, what lg_mlp_last_error returns), the device preamble and the weight upload of the create functions, and the widths of
// the opaque network handles, to check that the stages of an estimator fit together.
#pragma once
#include <hip/hip_runtime.h>
#include <string>
#include <vector>
#include "lg_device.h"
#include "../../include/lgpolicy.h"
#include "../../include/lgpolicy_wide.h"

// The exported entry point the caller called: the first line of every entry point that can fail is POLICY_ENTRY.  Entry points call each other
// (a collector calls the acts); the outermost name stays, so a message always begins with the call the caller made.
extern thread_local const char* lg_policy_entry;
struct PolicyEntry {
  bool outer;
  explicit PolicyEntry(const char* name) : outer(lg_policy_entry == nullptr) { if (outer) lg_policy_entry = name; }
  ~PolicyEntry() { if (outer) lg_policy_entry = nullptr; }
  PolicyEntry(const PolicyEntry&) = delete; PolicyEntry& operator=(const PolicyEntry&) = delete;
};
#define POLICY_ENTRY PolicyEntry entry_(__func__)

// records "<entry point>: <what>" as the thread's message and returns `status`, so a call site can return it
int lg_policy_fail(int status, const std::string& what);
#define POLICY_TRY(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) return lg_policy_fail(LG_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); } while (0)

// the preamble of a create function: a device exists and `device_id` names one; false + message otherwise.  The caller then opens its DeviceScope.
bool lg_policy_device_ok(int device_id);
// `bytes` of host memory in a fresh device allocation, registered in `allocs` (the owner's destroy frees those); NULL + message on failure
const void* lg_policy_upload(const void* host, size_t bytes, std::vector<void*>& allocs);

// the device a pointer lives on, -1 if it is not device memory: for the calls that take rows and no handle
int lg_policy_device_of(const void* p);

void lg_mlp_widths(const lg_mlp* m, int* layers, int* in, int* out, int* device);
void lg_rnn_widths(const lg_rnn* m, int* type, int* input, int* hidden, int* device);

// ---- the PPO collection loop (lg_policy.hip; mem_a NULL = the feed-forward ActorCritic): the one loop behind lg_collect_rollout,
// lg_collect_rollout_recurrent, lg_runner_collect and lg_runner_collect_privileged.  hooks NULL = a CollectHooks with nothing set.  Two modes:
//   one stream  (privileged_observations NULL): actor and critic read the same stored row, the env's (out->observations, O wide); `normalizer`
//               serves that row.  history, normalizer_c and last_observations are not read.
//   two streams (privileged_observations set): the critic reads the env's row (stored there, O_c wide, `normalizer_c`), the actor the history
//               layer's row or a column prefix of the env's raw row (out->observations, O_a wide, `normalizer`); a carried row each.
//   sensors     (one stream only) the env's step is lg_sensor_step_transition on this rig (include/lgsensors.h, lg_sensors.hip) in the place of
//               lg_step_transition: the ray caster between the step's two halves, the depth camera behind it.  Nothing else in the loop moves.
struct lg_obsnorm;
struct lg_sensor_rig;
// the rig's step behind its checks, and the context it is attached to (lg_sensors.hip)
int lg_policy_sensor_step(lg_sensor_rig* rig, const float* actions, float* next_obs, const float* values, float gamma, float* rewards, float* dones, void* stream);
lg_ctx* lg_policy_sensor_env(lg_sensor_rig* rig);
struct CollectHooks {
  lg_obsnorm* normalizer = nullptr;             // the actor's: every new row of its stream passes lg_obsnorm_step before it is stored and read; the row
                                                // after the last step is the handle's carried row, row 0 of the next collection
  lg_obsnorm* normalizer_c = nullptr;           // the critic's (two streams); both set: the paired step
  int update = 0;                               // the normalisers' training mode
  float* raw_rewards = nullptr;                 // (T, n): the env's rew_buf after each step
  float* extras = nullptr;                      // (T, K): the env's extras_episode after each step
  const lg_obs_history* history = nullptr;      // the actor's layer (two streams); NULL: the actor reads a column prefix of the env's row
  float* privileged_observations = nullptr;     // (T, n, O_c): selects the two-stream mode
  float* last_observations = nullptr;           // (n, O_a) or NULL: the actor's un-normalised row after the last step (two streams)
  lg_sensor_rig* sensors = nullptr;             // the env's sensor rig (one stream); NULL: the step is lg_step_transition
};
int lg_policy_collect_rollout(lg_ctx* env, lg_rnn* mem_a, lg_mlp* actor, lg_rnn* mem_c, lg_mlp* critic, const float* std, uint64_t seed, uint64_t first_call,
                              int32_t T, float gamma, float lam, int32_t normalize_advantage, const lg_rollout* out, const lg_rollout_hidden* hid, float* h_a,
                              float* c_a, float* h_c, float* c_c, const CollectHooks* hooks, void* stream);
// ---- the distillation collection loop (lg_policy.hip; recurrent = 0: the feed-forward StudentTeacher): the one loop behind
// lg_collect_distillation, lg_collect_distillation_recurrent, lg_runner_collect_distillation and lg_runner_collect_distillation_recurrent.
// hooks NULL = a DistillHooks with nothing set: the rows of the two plain collectors, launch for launch.  The teacher reads the env's row
// (out->privileged_observations, O_t wide, `normalizer_t`), the student the history layer's row or a column prefix of the env's raw row
// (out->observations, O_s wide, `normalizer_s`); a carried row each.  The four `*0` pointers take the memories' state before step 0.
struct DistillHooks {
  lg_obsnorm* normalizer_s = nullptr;           // the student's: every new row of its stream passes lg_obsnorm_step before it is stored and read; the row
                                                // after the last step is the handle's carried row, row 0 of the next collection
  lg_obsnorm* normalizer_t = nullptr;           // the teacher's; both set: the paired step
  int update = 0;                               // the normalisers' training mode
  float* raw_rewards = nullptr;                 // (T, n): the env's rew_buf after each step
  float* extras = nullptr;                      // (T, K): the env's extras_episode after each step
};
int lg_policy_collect_distillation(lg_ctx* env, int recurrent, lg_rnn* mem_s, lg_mlp* student, lg_rnn* mem_t, lg_mlp* teacher, const float* std, uint64_t seed,
                                   uint64_t first_call, int32_t T, const lg_obs_history* hist, const lg_distill_rollout* out, float* h_s0, float* c_s0, float* h_t0,
                                   float* c_t0, float* h_s, float* c_s, float* h_t, float* c_t, const DistillHooks* hooks, void* stream);
// the env's raw reward row (n) and episode-extras row (K): what the loop copies after each step, and the n of the runner's episode tail
struct EnvRewardRows { const float* rew = nullptr; const float* extras = nullptr; int64_t n = 0, K = 0; };
int lg_policy_reward_rows(lg_ctx* env, EnvRewardRows* rows);
// the carried row of a normaliser (lg_runner.hip): begin returns the (n, O) buffer (allocated on first use) and whether it holds a row, and marks it
// as not holding one; commit marks it as holding the row the collector left there
int lg_obsnorm_carried_begin(lg_obsnorm* h, int64_t n, int64_t O, float** row, bool* valid);
void lg_obsnorm_carried_commit(lg_obsnorm* h);
int lg_obsnorm_width(const lg_obsnorm* h);

// ---- the network handle, shared with the trainer (lg_train.hip), which rewrites the device buffers of an lg_mlp in place
#define MLP_ROWS 32          // batch rows per workgroup
#define MLP_THREADS 512      // eight waves: two per SIMD
#define MLP_MAXW 512         // widest layer; an input row may be wider (lg_mlp_create_wide: up to LG_MLP_MAX_INPUT), staged in slabs of this width
#define MLP_IMG (MLP_MAXW * MLP_ROWS)          // floats of one activation image
// element (row m, input k) of the activation image
#define IMG(m, k) (((((k) >> 4) * MLP_ROWS + (m)) * 4 + ((k) & 3)) * 4 + (((k) >> 2) & 3))

struct MlpDev {
  int L, act;
  int act_out;                       // != 0: the activation follows the last layer too (lg_mlp_set_output_activation); 0 for every network lg_mlp_create returns
  int dims[LG_MLP_MAX_LAYERS + 1];
  int kpad[LG_MLP_MAX_LAYERS];       // input width rounded up to 64 (four blocks of four k-steps of 4)
  int nchunks[LG_MLP_MAX_LAYERS];    // output width rounded up to 16, / 16
  const float* w[LG_MLP_MAX_LAYERS]; // tiled weights [chunk][k/16][lane][4]
  const float* b[LG_MLP_MAX_LAYERS]; // bias, padded to 16 * nchunks
};

struct lg_mlp {
  MlpDev h;
  int device = 0;
  std::vector<void*> allocs;
};
// a handle whose input row does not fit one activation image: its launches take the kernels' wide instances (split-K first layer)
inline bool mlp_is_wide(const lg_mlp* m) { return m->h.kpad[0] > MLP_MAXW; }

// the activations, shared so that the trainer's forward values are lg_mlp_forward's bit for bit
LG_DEV float apply_act(float x, int act) {
  switch (act) {
    case LG_ACT_ELU: {   // x > 0 ? x : expm1(x): the degree-6 Taylor polynomial for -0.25 < x < 0 (truncation x^7 / 5040 < 1.3e-8), exp(x) - 1
                         // from -0.25 down (fast exp, on a result of magnitude >= 0.22); libm's expm1f is ~30 instructions.  Measured against
                         // float64 on MI355X over 5232 points in [-30, 30] (tests/test_hip_policy_sweep.py): polynomial 2.2e-8 absolute
                         // (1.0e-7 relative), exp branch 4.8e-8 absolute (6.9e-8 relative) -- torch's fp32 ELU on the CPU: 4.7e-8 --, and
                         // monotone across the switch: the step from -0.25 to the next float is 3.0e-8 where float64 has 1.2e-8
      const float p = x * (1.f + x * (0.5f + x * (1.f / 6 + x * (1.f / 24 + x * (1.f / 120 + x * (1.f / 720))))));
      return x > 0.f ? x : (x > -0.25f ? p : __expf(x) - 1.f);
    }
    case LG_ACT_RELU: return fmaxf(x, 0.f);
    case LG_ACT_TANH: return tanhf(x);
    case LG_ACT_LRELU: return x > 0.f ? x : 0.01f * x;
    case LG_ACT_SELU: return 1.0507009873554805f * (x > 0.f ? x : 1.6732632423543772f * expm1f(x));
  }
  return x;
}

// ---- the memory handle, shared with the recurrent trainer (lg_train_recurrent.hip), which rewrites the device images of an lg_rnn in place
#define RNN_KMAX 1024        // widest concatenated row: 512 inputs + 512 hidden, each padded to 16
#define RNN_MAX_LAYERS 4

struct RnnLayerDev {
  int gru, I, H, Ip, nbx, nb, nch;   // Ip: x padded to 16; nbx = Ip / 16 blocks of x, nb blocks of [x ; h]; nch chunks of 16 hidden units
  const float* w;                    // tiled [chunk][block][gate][lane][4]
  const float* b;                    // [4][16 * nch]: LSTM b_ih + b_hh of i f g o; GRU (b_ir + b_hr), (b_iz + b_hz), b_in, b_hn
};

struct lg_rnn {
  int type = 0, num_layers = 0, input = 0, hidden = 0, device = 0;
  RnnLayerDev layer[RNN_MAX_LAYERS];
  std::vector<void*> allocs;
  // a wide memory (lg_rnn_create_wide, more than RNN_XMAX inputs): layer 0 is two launches.  rnn_wide_xproj_kernel walks the x part of the chain
  // over `xproj` (w: [chunk][nbx + 1 blocks][gate][lane][4], the last block zero; I, Ip, nbx, nch, H as usual; b unused) into y, and the seeded tile
  // (lg_rnn_tile.h, SEED) goes on over layer[0], which then describes the h part alone: I = Ip = nbx = 0, nb = nch.
  bool wide = false;
  RnnLayerDev xproj{};
  float* y = nullptr;                // (y_rows, G * 16 nch): the projection of the last step, owned; grows with n, never shrinks
  int64_t y_rows = 0;
  hipStream_t y_stream = nullptr;    // the stream y was last used on: drained before y is released
};
#define RNN_XMAX 512         // widest input of the one-launch layer (RNN_KMAX - 512); a slab of the projection's staged row
// The x part of a wide layer 0 for rows [0, n): y[(row * G + g) * Hp + u] = sum_k x[src(row)][k] w_ih[g H + u][k], ONE k-ascending chain per output over
// blocks of 16 inputs (the order rnn_blocks walks the x part of the narrow layer), src(row) = idx ? idx[row] : row.  b NULL: one memory.
struct RnnXprojArgs { RnnLayerDev L; const float* x; const int64_t* idx; float* y; };
void rnn_launch_xproj(const RnnXprojArgs* a, const RnnXprojArgs* b, int64_t n, hipStream_t st);
// [chunk][nb + 1 blocks][gate][lane][4] of Wcat[:, 0 .. I) = w_ih, Wcat[:, Ip .. Ip + H) = w_hh (either may be absent: I = 0, or Ip past the last block)
void rnn_tile_weights_at(int G, int I, int Ip, int nb, int H, const float* w_ih, const float* w_hh, float* tiled);
#define RNN_NO_HH (1 << 30)  // the Ip of an image without a hidden part
