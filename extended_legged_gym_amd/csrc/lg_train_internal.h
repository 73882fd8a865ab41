// lg_train_internal.h — what the trainers share (lg_train.hip: PPO over two networks; lg_distill_train.hip: distillation over one;
// lg_train_recurrent.hip: PPO over two networks behind two memories; lg_train_symmetry.hip: PPO with symmetry tables, its own staging kernels): the
// description of a network and of a (network, layer) segment as the kernels of lg_train.hip see them, the scalars the optimiser keeps on the
// device, and the host calls that size the workspaces and launch those kernels.  The kernels themselves live in lg_train.hip only.  So do the bodies
// of the entry points every trainer exports under its own prefix (train_api_*, at the end of this file).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <vector>
#include "lg_device.h"
#include "lg_policy_internal.h"
#include "../../include/lgtrain.h"

#define WGRAD_SLAB 256        // batch rows per slab of the weight-gradient pass
#define TRAIN_MAX_NETS 2
// the layers of two MLPs, and weight_ih / weight_hh of every layer of two memories (lg_train_recurrent.hip)
#define TRAIN_MAX_SEGS (TRAIN_MAX_NETS * LG_MLP_MAX_LAYERS + TRAIN_MAX_NETS * 2 * RNN_MAX_LAYERS)

// one network as the forward and the backward tile see it
struct TrainNet {
  int L, act;
  int dims[LG_MLP_MAX_LAYERS + 1];
  int fkpad[LG_MLP_MAX_LAYERS], fnch[LG_MLP_MAX_LAYERS];   // forward tiling of layer l (the lg_mlp's): padded input width, 16-column chunks
  int bkpad[LG_MLP_MAX_LAYERS], bnch[LG_MLP_MAX_LAYERS];   // transposed tiling of layer l: dims[l + 1] padded to 64, chunks of dims[l] padded to 64
  const float* fw[LG_MLP_MAX_LAYERS];
  const float* fb[LG_MLP_MAX_LAYERS];
  const float* bw[LG_MLP_MAX_LAYERS];                      // layer 0 has none unless its owner adds one (the recurrent trainer): nothing is propagated into observations
  float* a[LG_MLP_MAX_LAYERS + 1];                         // a[l] (rows, dims[l]): output of layer l - 1; a[L] is the network's output; a[0] unused
  float* d[LG_MLP_MAX_LAYERS];                             // d[l] (rows, dims[l + 1]): dL / d(pre-activation output of layer l)
};

// one (network, layer) of the weight-gradient, reduce and Adam passes; element e of a segment is (o, i) = (e / (dI + 1), e % (dI + 1)), i == dI the bias
struct TrainSeg {
  int net, layer, dO, dI;
  int f_nb, b_nb;                    // 16-input blocks per chunk of the forward / transposed tiling
  int64_t woff, boff;                // offsets of W and b in the flat parameter vector
  const float* D;                    // (rows, dO)
  const float* Ain;                  // (rows, dI); NULL: the gathered observation rows
  float* partial;                    // [slab][dO][dI + 1]
  float* fw; float* fb; float* bw;    // fw / fb NULL: a segment whose forward image is not an lg_mlp's (a memory's: the owner rewrites it itself)
};

struct TrainScalars {
  double lr;
  double acc[4];                     // sums over an update's steps: value, surrogate, entropy, KL
  float means[4];                    // last mini-batch: surrogate, value, entropy, KL
  float norm, clip, step_size, bc2_sqrt;
  int64_t step;
};

// The networks, their segments, the masters with Adam's moments and the workspaces for up to max_rows rows.  The flat parameter vector is the
// networks' tensors in order (W0, b0, W1, b1, ...) and then nstd trailing floats at std_off (PPO's std / log_std; none for distillation).
struct TrainCore {
  int device = 0, nnet = 0, nseg = 0;
  int nstd = 0, std_type = 0;
  int64_t max_rows = 0, P = 0, std_off = 0, last_rows = 0, big = 0;
  int red_blocks = 0, wgrad_blocks = 1;
  TrainNet net[TRAIN_MAX_NETS];
  TrainSeg seg[TRAIN_MAX_SEGS];
  TrainSeg* d_seg = nullptr;
  float *theta = nullptr, *m = nullptr, *v = nullptr, *G = nullptr, *norm_part = nullptr, *std_dev = nullptr;
  TrainScalars* sc = nullptr;
  std::vector<void*> allocs;
  // the trainers that run groups of steps: the step losses of the last group and of the last update (train_api_group_gradients / _step_losses)
  int64_t last_steps = 0, last_update_steps = 0;
  float *group_loss = nullptr, *seq_loss = nullptr;
  // the owner's own images of the masters (a memory's, a convolution's), rewritten after set_state; NULL: the core's tilings are all there is
  int (*retile_own)(TrainCore*, hipStream_t) = nullptr;
};

// fixed-order tree over the 256 lanes of a block
LG_DEV float block_sum_256(float x, float* red) {
  const int tid = threadIdx.x;
  red[tid] = x;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) { if (tid < off) red[tid] += red[tid + off]; __syncthreads(); }
  return red[0];
}

typedef float f32x4 __attribute__((ext_vector_type(4)));

// one 16-column chunk over nblk blocks of 16 inputs: both row halves, k ascending (the chain order of mlp_tile)
LG_DEV void chunk_chain(const float4* __restrict__ wc, const float4* ap, int nblk, f32x4& acc0, f32x4& acc1) {
  for (int kb = 0; kb < nblk; ++kb) {
    const float4 w = wc[(size_t)kb * 64], p = ap[kb * 128], q = ap[kb * 128 + 64];
    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(p.x, w.x, acc0, 0, 0, 0); acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(q.x, w.x, acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(p.y, w.y, acc0, 0, 0, 0); acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(q.y, w.y, acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(p.z, w.z, acc0, 0, 0, 0); acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(q.z, w.z, acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(p.w, w.w, acc0, 0, 0, 0); acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(q.w, w.w, acc1, 0, 0, 0);
  }
}

// a device allocation the core owns (train_core_free releases it); NULL + message on failure
void* train_alloc(TrainCore* c, size_t bytes, bool zero);
// appends `net`: its transposed tilings, the activation / delta workspaces for c->max_rows rows, one segment per layer at offset *off of the flat
// vector (advanced).  false + message on failure.
bool train_core_add_net(TrainCore* c, const lg_mlp* net, int64_t* off);
// appends one dense segment that is no layer of an lg_mlp (a memory's weight_ih / weight_hh, a linear layer of another stage): its slab partials for
// c->max_rows rows; the owner places it in the flat vector (woff / boff) itself.  *ok goes false (+ message) on failure.
TrainSeg& train_core_add_seg(TrainCore* c, int net, int layer_id, int dO, int dI, const float* D, const float* Ain, float* fw, float* fb, int f_nb, float* bw, int b_nb,
                             bool* ok);
// after the networks: c->P = off + c->nstd; masters, moments, gradient, norm partials, scalars, the device copy of the segments; uploads the masters
// from HOST weights / biases per network in torch's layout (+ tail: the nstd trailing floats) and writes every tiling from them.
int train_core_finish(TrainCore* c, int64_t off, const float* const* const* weights, const float* const* const* biases, const float* tail, double learning_rate);
void train_core_free(TrainCore* c);

// forward with saved activations over the rows obs[idx[0 .. n)] (cobs: the second network's rows), and the backward data pass from d[L - 1]
void train_launch_forward(const TrainCore* c, const float* obs, const float* cobs, const int64_t* idx, int64_t n, hipStream_t st);
void train_launch_backward(const TrainCore* c, int64_t n, hipStream_t st);
// the backward data pass of network k alone, for a trainer whose networks do not share a row count (lg_train_symmetry.hip)
void train_launch_backward_net(const TrainCore* c, int k, int64_t n, hipStream_t st);
// weight gradients by slabs, their reduction, the global norm (clip_on == 0: the norm is reported and the gradient passes unscaled), Adam and the
// rewrite of the tilings.  idx must not be NULL.
int train_launch_optimise(TrainCore* c, const float* obs, const float* cobs, const int64_t* idx, int64_t n, float max_grad_norm, int clip_on, hipStream_t st);
// the same passes one by one over segments [seg0, seg0 + count): the slab weight gradients of dense segments over n rows; the reduction of nslabs
// partials (any kernel may have written them, in the layout of TrainSeg::partial); then, once every segment is reduced, norm + Adam + tilings
void train_launch_wgrad_range(const TrainCore* c, int seg0, int count, const float* obs, const float* cobs, const int64_t* idx, int64_t n, hipStream_t st);
void train_launch_reduce_range(const TrainCore* c, int seg0, int count, int nslabs, hipStream_t st);
int train_launch_norm_adam(TrainCore* c, float max_grad_norm, int clip_on, hipStream_t st);
// the masters -> the tilings (and std_dev), without a step
int train_core_retile(TrainCore* c, hipStream_t st);

// The whole body of the entry points every trainer exports as <prefix>_parameter_count / _workspace_bytes / _get_state / _get_parameters / _set_state /
// _set_learning_rate: the checks with their messages, the device scope, the copies and the final synchronise.  An exported function is POLICY_ENTRY
// and one call, so a refusal names the entry point the caller called.  c may be NULL (refused).
int64_t train_api_parameter_count(TrainCore* c);
int64_t train_api_workspace_bytes(TrainCore* c);
int train_api_get_state(TrainCore* c, float* params, float* exp_avg, float* exp_avg_sq, int64_t* step, double* lr, void* stream);
int train_api_get_parameters(TrainCore* c, float* params, void* stream);
int train_api_set_state(TrainCore* c, const float* params, const float* exp_avg, const float* exp_avg_sq, int64_t step, double lr, void* stream);
int train_api_set_learning_rate(TrainCore* c, double lr, void* stream);
// <prefix>_gradients / _step_losses of the trainers that run groups of steps: the gradient, the norm the clip used and the last group's step losses
// (last_steps of group_loss); the first `count` of the last update's last_update_steps losses in seq_loss
int train_api_group_gradients(TrainCore* c, float* g, float* norm, float* losses, int64_t capacity, void* stream);
int train_api_step_losses(TrainCore* c, float* losses, int64_t count, void* stream);

// PPO's clipped losses on the mini-batch rows i (rollout rows idx[i]) from the forward outputs a[L] of networks 0 and 1: dL/dmu and dL/dvalue into
// d[L - 1], the four loss means and the gradient of std / log_std (into G at std_off), the KL-adaptive learning rate.  loss_part: the caller's
// train_ppo_loss_floats(max_rows) floats.
size_t train_ppo_loss_floats(int64_t max_rows);
void train_launch_ppo_loss(TrainCore* c, const lg_ppo_rows* rows, const int64_t* idx, int64_t n, const lg_ppo_hyper* hyper, float* loss_part, int accumulate, hipStream_t st);
// mode 0: clear the update's sums; 1: the means over `steps` steps and the learning rate -> stats (device)
void train_launch_ppo_stats(TrainCore* c, lg_ppo_stats* stats, int mode, int steps, hipStream_t st);
